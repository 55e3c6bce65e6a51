"""The forward-only objective (rae_eval_cost, TrainEngine.evaluate, func['cost_<split>']) on an
MI355X against the float64 oracle / the reference's golden vectors.

Reference: oracle/rae_oracle.py train_step_grads(...).scores and .cost at the device's own
parameters cast to float64, with the device's own negative arrays read back.  Per example
  pos = scores[:l] + scores[l:2l],  H = scores[2l:3l],
  neg = scores[4l:] reshaped (2s, l) summed over axis 0 for 'sp', (2, l, s) summed over axes 0
        and 2 for the bilinear decoders.
Tolerances (the project's own): cost |dc| <= 2e-5 max(1, |c|) (COST_RTOL); per-example terms
rtol 1e-4, atol 1e-5 (test_forward_launch_alone_vs_oracle's bounds for forward quantities).
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import rae_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

COST_RTOL = 2e-5
TERM_RTOL, TERM_ATOL = 1e-4, 1e-5

SP_CASES = ["sp_basic", "sp_reg", "sp_sgd_noext"]
BIL_CASES = ["rescal_basic", "rescal_reg", "hybrid_basic", "hybrid_testpy"]


# ----------------------------------------------------------------------------------- helpers
def _case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    X = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=(int(z["N"]), int(z["d"])))
    return z, X


def _golden_inducer(z, X, dev, **kw):
    from rae.data import DatasetManager, DatasetSplit
    from rae.inducer import ReconstructInducer
    data = DatasetManager({"train": DatasetSplit(z["args1"], z["args2"], X)}, z["freqs"],
                          int(z["d"]))
    rng = np.random.RandomState(int(z["seed"]))
    return ReconstructInducer(data, {"train": {}}, rng, int(z["epochs"]), float(z["lr"]),
                              int(z["l"]), int(z["r"]), int(z["m"]), int(z["s"]), float(z["l1"]),
                              float(z["l2"]), str(z["optimizer"]), "golden", str(z["decoder"]),
                              False, bool(int(z["ext_reg"])), False, float(z["alpha"]),
                              device=dev, **kw)


def _inducer(data, gold, dev, dec, m, r, s, l, epochs=1, seed=2, **kw):
    from rae.inducer import ReconstructInducer
    return ReconstructInducer(data, gold, np.random.RandomState(seed), epochs, 0.1, l, r, m, s,
                              0.0, 0.0, "adagrad", "ev", dec, False, True, False, 1.0,
                              device=dev, graph_chunk=2, **kw)


def _params(ind):
    return {k: v.detach().cpu().double().numpy() for k, v in ind.modelFunc.named_params().items()}


def _group(dec, scores, l, s):
    """(pos, H, neg) per example from the reference's all_scores vector."""
    pos = scores[:l] + scores[l:2 * l]
    H = scores[2 * l:3 * l]
    negs = scores[4 * l:]
    if dec == "sp":
        neg = negs.reshape(2 * s, l).sum(axis=0)
    else:
        neg = negs.reshape(2, l, s).sum(axis=(0, 2))
    return np.stack([pos, H, neg], axis=1)


def _oracle(dec, params, split, rows, n1, n2, alpha=1.0):
    """Oracle terms (nrows, 3) and cost of `rows` (a slice) of a host split; n1 / n2 (s, nrows)."""
    X = split.xFeats[rows]
    a1, a2 = split.args1[rows], split.args2[rows]
    res = O.train_step_grads(dec, params, X, a1, a2, np.asarray(n1), np.asarray(n2), alpha=alpha)
    return _group(dec, res.scores, len(a1), n1.shape[0]), res.cost


def _check(res, want_terms, want_cost, what=""):
    got = res.terms.cpu().double().numpy()
    err = np.abs(got - want_terms)
    print(f"{what}: max |dterm| {err.max():.3e} (|term| max {np.abs(want_terms).max():.3e}), "
          f"cost {res.cost:.9f} oracle {want_cost:.9f} |dc| {abs(res.cost - want_cost):.3e}")
    np.testing.assert_allclose(got, want_terms, rtol=TERM_RTOL, atol=TERM_ATOL, err_msg=what)
    assert abs(res.cost - want_cost) <= COST_RTOL * max(1.0, abs(want_cost)), (what, res.cost,
                                                                               want_cost)


def _randomize(ind, seed=0):
    """Parameters far from the (nearly uniform-P) initial point."""
    import torch
    g = np.random.RandomState(seed)
    scale = {"W": 0.4, "Wb": 0.5, "A": 0.5, "Ab": 0.5}
    for k, v in ind.modelFunc.named_params().items():
        x = g.standard_normal(tuple(v.shape)) * scale.get(k, 0.3)
        v.copy_(torch.as_tensor(x.astype(np.float32)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. golden, all fixtures
@pytest.mark.parametrize("name", SP_CASES + BIL_CASES)
def test_golden_step0_terms_and_cost(built_lib, cuda_dev, name):
    z, X = _case(name)
    ind = _golden_inducer(z, X, cuda_dev)
    ind.compile_function()
    l, s, dec = int(z["l"]), int(z["s"]), str(z["decoder"])
    res = ind.engine.evaluate(ind.engine.split, 0, l, z["neg1_e0"][:, :l], z["neg2_e0"][:, :l],
                              terms=True)
    want = _group(dec, z["step0_scores"], l, s)
    np.testing.assert_allclose(want[:, 1], z["step0_H"], rtol=0, atol=1e-15)
    got = res.terms.cpu().double().numpy()
    np.testing.assert_allclose(got, want, rtol=TERM_RTOL, atol=TERM_ATOL)
    np.testing.assert_allclose(got[:, 1], z["step0_H"], rtol=TERM_RTOL, atol=TERM_ATOL)
    c = -float(np.mean(z["step0_scores"]))
    assert abs(res.cost - c) <= COST_RTOL * max(1.0, abs(c)), (res.cost, c)
    assert abs((res.reconstruction + res.entropy) - res.cost) <= 1e-12


# --------------------------------------------------------------- 2. synthetic vs the oracle
SYN = [
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="sp"),            # scalar paths
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="rescal"),
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="rescal+sp"),
    dict(N=300, d=2000, m=100, r=200, s=20, ntrue=10, dec="sp"),      # headline K/r/s
    dict(N=300, d=400, m=8, r=16, s=36, ntrue=4, dec="sp"),
    dict(N=300, d=400, m=8, r=300, s=4, ntrue=4, dec="sp"),
    dict(N=300, d=800, m=200, r=16, s=4, ntrue=6, dec="sp"),
    dict(N=200, d=2000, m=100, r=200, s=20, ntrue=10, dec="rescal"),  # C5 shape
    dict(N=200, d=1000, m=30, r=60, s=10, ntrue=6, dec="rescal+sp"),
    dict(N=64, d=3000, m=300, r=300, s=50, ntrue=10, dec="sp"),       # C4 K/r/s
]


@pytest.mark.parametrize("shape", SYN, ids=lambda p: f"{p['dec']}-m{p['m']}-r{p['r']}-s{p['s']}")
def test_synthetic_vs_oracle(built_lib, cuda_dev, shape):
    from rae.data import synthetic_dataset
    data, gold = synthetic_dataset(shape["N"], shape["d"], shape["ntrue"], seed=99)
    dec, N = shape["dec"], shape["N"]
    ind = _inducer(data, gold, cuda_dev, dec, shape["m"], shape["r"], shape["s"], min(50, N))
    ind.compile_function()
    eng = ind.engine
    rng_state = ind.rng.get_state()
    n1, n2 = eng.eval_negatives(eng.split, ind.negativeSampler)
    assert tuple(n1.shape) == (shape["s"], N) and not bool((n1 == n2).all())
    res = eng.evaluate(eng.split, terms=True)
    want, cost = _oracle(dec, _params(ind), data.split["train"], slice(0, N),
                         n1.cpu().numpy(), n2.cpu().numpy())
    _check(res, want, cost, str(shape))
    # cached: the same arrays every time; the model's RNG stream is untouched
    m1, m2 = eng.eval_negatives(eng.split, ind.negativeSampler)
    assert m1.data_ptr() == n1.data_ptr() and m2.data_ptr() == n2.data_ptr()
    st = ind.rng.get_state()
    assert st[2] == rng_state[2] and np.array_equal(st[1], rng_state[1])


# --------------------------------------------------------------------- 3. after training
def _three_splits(N=800, d=300, ntrue=4, seed=31, cut=(400, 600)):
    from rae.data import DatasetManager, DatasetSplit, synthetic_dataset
    full, _ = synthetic_dataset(N, d, ntrue, seed=seed)
    tr = full.split["train"]
    n = full.get_arg_voc_size()
    a, b = cut
    mk = lambda lo, hi: DatasetSplit(tr.args1[lo:hi], tr.args2[lo:hi], tr.xFeats[lo:hi])
    data = DatasetManager.from_arrays(tr.xFeats[:a], tr.args1[:a], tr.args2[:a], n_entities=n,
                                      n_features=d, valid=mk(a, b), test=mk(b, N))
    return data, {"train": {}, "valid": {}, "test": {}}


@pytest.mark.parametrize("dec", ["sp", "rescal"])
def test_held_out_split_after_training(built_lib, cuda_dev, dec):
    import torch
    data, gold = _three_splits()
    ind = _inducer(data, gold, cuda_dev, dec, 8, 16, 4, 50, epochs=1)
    ind.learn(verbose=False)
    torch.cuda.synchronize()
    eng = ind.engine
    vs = ind._dev_split["valid"]
    res = eng.evaluate(vs, terms=True)
    n1, n2 = eng.eval_negatives(vs)
    want, cost = _oracle(dec, _params(ind), data.split["valid"], slice(0, vs.N),
                         n1.cpu().numpy(), n2.cpu().numpy())
    _check(res, want, cost, f"valid after training, {dec}")
    assert res.terms.shape[0] == 200


# -------------------------------------------------------------------------------- 4. edges
EDGE_NNZ = [0, 1, 17, 64, 65, 130]


@pytest.fixture(scope="module")
def edge_data():
    from rae.data import DatasetManager
    g = np.random.RandomState(4)
    N, d, n = 70, 400, 30
    nnz = np.array(EDGE_NNZ + list(g.randint(1, 12, size=N - len(EDGE_NNZ))))
    rows = np.repeat(np.arange(N), nnz)
    cols = np.concatenate([g.choice(d, size=k, replace=False) for k in nnz]).astype(np.int64)
    vals = g.uniform(0.25, 1.75, size=rows.shape[0]).astype(np.float32)     # non-binary values
    X = sp.csr_matrix((vals, (rows, cols)), shape=(N, d))
    a1 = g.randint(0, n, N).astype(np.int32)
    a2 = g.randint(0, n, N).astype(np.int32)
    a1[:n] = np.arange(n)                       # every entity seen
    a2[3] = a1[3]                               # e1 == e2
    data = DatasetManager.from_arrays(X, a1, a2, n_entities=n, n_features=d)
    s, stride = 3, N + 7                        # neg_stride > row0 + nrows
    n1 = g.randint(0, n, size=(s, stride)).astype(np.int32)
    n2 = g.randint(0, n, size=(s, stride)).astype(np.int32)
    n1[0, 5] = a1[5]                            # a negative equal to e1
    n2[1, 5] = a1[5]
    n1[:, 6] = n1[0, 6]                         # duplicate negatives
    n2[:, 7] = n2[0, 7]
    return data, n1, n2


@pytest.mark.parametrize("dec", ["sp", "rescal", "rescal+sp"])
def test_edges(built_lib, cuda_dev, edge_data, dec):
    data, n1, n2 = edge_data
    split = data.split["train"]
    assert list(np.diff(split.xFeats.indptr)[:6]) == EDGE_NNZ
    ind = _inducer(data, {"train": {}}, cuda_dev, dec, 12, 20, 3, 10)
    ind.compile_function()
    _randomize(ind, seed=3)
    eng = ind.engine
    assert eng.split.values is not None
    N = eng.split.N
    want_all, _ = _oracle(dec, _params(ind), split, slice(0, N), n1[:, :N], n2[:, :N])
    for row0, nrows in ((0, N), (0, 1), (0, 15), (0, 17), (0, 65), (2, 1), (3, 17), (5, 65),
                        (69, 1), (7, 0)):
        res = eng.evaluate(eng.split, row0, nrows, n1, n2, terms=True)
        want = want_all[row0:row0 + nrows]
        S = want.sum(axis=0)
        cost = -(S[0] + 2 * S[1] + S[2]) / (nrows * (4 + 2 * 3)) if nrows else 0.0
        if nrows == 0:
            assert res.sums == (0.0, 0.0, 0.0) and res.cost == 0.0 and res.terms.shape == (0, 3)
            continue
        _check(res, want, cost, f"{dec} rows [{row0}, {row0 + nrows})")
    # the oracle's own cost of one range, as a cross-check of the cost formula above
    w, c = _oracle(dec, _params(ind), split, slice(3, 20), n1[:, 3:20], n2[:, 3:20])
    res = eng.evaluate(eng.split, 3, 17, n1, n2, terms=True)
    _check(res, w, c, f"{dec} rows [3, 20) vs the oracle's cost")


# ------------------------------------------------------------ 5. tiling independence, bitwise
@pytest.mark.parametrize("shape", [
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="sp"),
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="rescal"),
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="rescal+sp"),
    dict(N=200, d=2000, m=100, r=200, s=20, ntrue=10, dec="rescal"),
], ids=lambda p: f"{p['dec']}-m{p['m']}")
def test_terms_do_not_depend_on_the_range(built_lib, cuda_dev, shape):
    import torch
    from rae.data import synthetic_dataset
    data, gold = synthetic_dataset(shape["N"], shape["d"], shape["ntrue"], seed=99)
    ind = _inducer(data, gold, cuda_dev, shape["dec"], shape["m"], shape["r"], shape["s"], 50)
    ind.compile_function()
    _randomize(ind, seed=5)
    eng, N = ind.engine, shape["N"]
    eng.eval_negatives(eng.split, ind.negativeSampler)
    whole = eng.evaluate(eng.split, terms=True)
    part = eng.evaluate(eng.split, 37, 50, terms=True)
    assert torch.equal(part.terms, whole.terms[37:87])
    again = eng.evaluate(eng.split, terms=True)
    assert again.sums == whole.sums and torch.equal(again.terms, whole.terms)
    want = whole.terms.double().sum(dim=0).cpu().numpy()
    for got, w in zip(whole.sums, want):
        assert abs(got - w) <= 1e-12 * abs(w), (got, w)
    # without the terms output the sums are the same (the terms then live in the workspace)
    assert eng.evaluate(eng.split).sums == whole.sums


# --------------------------------------------------------------------- 6. nothing else moves
@pytest.mark.parametrize("dec", ["sp", "rescal"])
def test_eval_cost_leaves_training_untouched(built_lib, cuda_dev, dec):
    import torch
    from rae.data import synthetic_dataset
    runs = []
    for on in (True, False, True):
        data, gold = synthetic_dataset(400, 300, 4, seed=31)
        ind = _inducer(data, gold, cuda_dev, dec, 8, 16, 4, 50, epochs=2, eval_cost=on)
        ind.learn(verbose=False)
        torch.cuda.synchronize()
        acc = [v.detach().cpu().numpy() for v in ind.optimizer.accumulator]
        runs.append((list(ind.train_errors), _params(ind), acc, ind.rng.get_state(),
                     list(ind.eval_costs["train"])))
    on, off, on2 = runs
    assert on[0] == off[0]
    for k in on[1]:
        assert np.array_equal(on[1][k], off[1][k]), k
    for x, y in zip(on[2], off[2]):
        assert np.array_equal(x, y)
    assert on[3][2] == off[3][2] and np.array_equal(on[3][1], off[3][1])
    assert len(on[4]) == 2 and off[4] == [] and all(np.isfinite(on[4]))
    assert on[4] == on2[4]


# ------------------------------------------------------- 7. func['cost_train'] vs func['train']
@pytest.mark.parametrize("name", ["sp_basic", "rescal_basic", "hybrid_basic"])
def test_cost_train_matches_func_train(built_lib, cuda_dev, name):
    z, X = _case(name)
    assert float(z["l1"]) == 0.0 and float(z["l2"]) == 0.0
    ind = _golden_inducer(z, X, cuda_dev)
    ind.compile_function()
    l = int(z["l"])
    n1, n2 = z["neg1_e0"][:, :l], z["neg2_e0"][:, :l]
    want = float(z["costs"][0, 0])
    c_eval = ind.func["cost_train"](0, n1, n2)
    assert abs(c_eval - want) <= COST_RTOL * max(1.0, abs(want)), (c_eval, want)
    for k, v in _params(ind).items():                 # the call changed nothing
        assert np.array_equal(v, z["init_" + k].astype(np.float32).astype(np.float64)), k
    c_train = ind.func["train"](0, n1, n2)
    print(f"{name}: cost_train {c_eval:.9f} train {c_train:.9f} diff {abs(c_eval - c_train):.3e}")
    assert abs(c_eval - c_train) <= 2e-6, (c_eval, c_train)
    # a later batch: func['train']'s slicing (rows [b l, (b+1) l), per-call negative columns)
    b = 1
    p = _params(ind)
    c1 = ind.func["cost_train"](b, z["neg1_e0"][:, b * l:(b + 1) * l],
                                z["neg2_e0"][:, b * l:(b + 1) * l])
    from rae.data import DatasetSplit
    _, oc = _oracle(str(z["decoder"]), p, DatasetSplit(z["args1"], z["args2"], X),
                    slice(b * l, (b + 1) * l), z["neg1_e0"][:, b * l:(b + 1) * l],
                    z["neg2_e0"][:, b * l:(b + 1) * l], alpha=float(z["alpha"]))
    assert abs(c1 - oc) <= COST_RTOL * max(1.0, abs(oc)), (c1, oc)


# ------------------------------------------------------------------- 8. mode 2 end to end
def test_mode2_reports_held_out_objective(built_lib, cuda_dev, capsys):
    data, gold = _three_splits()
    ind = _inducer(data, gold, cuda_dev, "sp", 8, 16, 4, 50, epochs=1, eval_cost=True)
    ind.learn(verbose=True)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if " objective: " in ln]
    assert [ln.split()[0] for ln in lines] == ["valid", "test"], out
    assert all("reconstruction" in ln and "entropy" in ln for ln in lines)
    assert len(ind.eval_costs["valid"]) == 1 and len(ind.eval_costs["test"]) == 1
    assert ind.eval_costs["train"] == []
    assert all(np.isfinite(ind.eval_costs[k][0]) for k in ("valid", "test"))
    # off: no objective line, nothing recorded
    ind2 = _inducer(data, gold, cuda_dev, "sp", 8, 16, 4, 50, epochs=1)
    ind2.learn(verbose=True)
    out2 = capsys.readouterr().out
    assert " objective: " not in out2 and ind2.eval_costs["valid"] == []


# ------------------------------------------------------------------- 9. stream-ordered call
@pytest.mark.parametrize("shape", [
    dict(N=64, d=3000, m=300, r=300, s=50, ntrue=10, dec="sp"),       # > 48 KiB of LDS per tile
    dict(N=210, d=700, m=7, r=13, s=3, ntrue=5, dec="rescal+sp"),
], ids=lambda p: f"{p['dec']}-m{p['m']}")
def test_eval_cost_is_graph_capturable(built_lib, cuda_dev, shape):
    """rae_eval_cost allocates nothing and never synchronises: it can be captured into a HIP
    graph (like rae_label) and the replay gives the eager call's terms and sums bit for bit."""
    import torch
    from rae.data import synthetic_dataset
    data, gold = synthetic_dataset(shape["N"], shape["d"], shape["ntrue"], seed=99)
    ind = _inducer(data, gold, cuda_dev, shape["dec"], shape["m"], shape["r"], shape["s"], 32)
    ind.compile_function()
    eng, N = ind.engine, shape["N"]
    n1, n2 = eng.eval_negatives(eng.split, ind.negativeSampler)
    eager = eng.evaluate(eng.split, terms=True)
    out = torch.zeros((N, 3), dtype=torch.float32, device=cuda_dev)
    eng._eval_sums.zero_()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(cuda_dev)
    s.wait_stream(torch.cuda.current_stream(cuda_dev))
    with torch.cuda.graph(g, stream=s):
        eng.queue_evaluate(eng.split, 0, N, n1, n2, out)
    torch.cuda.current_stream(cuda_dev).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager.terms)
    assert tuple(float(x) for x in eng._eval_sums.cpu().numpy()) == eager.sums
