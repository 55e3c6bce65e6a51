"""Cluster evaluation on the device (rae_cluster_count / rae_b3_metrics, include/rae.h;
TrainEngine.cluster_metrics; ReconstructInducer(cluster_eval="device")) against the array
oracle of rae/evaluation.py (contingency_table, b3_from_table), which tests/test_cluster_host.py
pins to the reference-executed evaluator."""
import ctypes as C
import types
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# csrc/rae_cluster.hpp: 256 threads, the grid sized for 4 row quads per thread, at most 512
# workgroups in the LDS form -- past this many rows a thread's grid-strided loop runs on
GRID_CAP_ROWS_LDS = 512 * 256 * 4 * 4
SIZES = [0, 1, 63, 64, 65, 255, 257, 1023, 4097, 70001]
SHAPES = [(1, 0), (3, 1), (100, 7), (100, 41), (512, 127), (512, 4095)]


def _gi(ids, ng):
    """A GoldIndex stand-in over raw gold ids (contingency_table reads ids / n_gold / n_rows)."""
    ids = np.asarray(ids, dtype=np.int32)
    return types.SimpleNamespace(ids=ids, n_gold=int(ng), n_rows=int(ids.shape[0]))


def _p(t):
    """The tensor's device address (from its storage: an empty view's data_ptr() is 0)."""
    if t is None:
        return None
    return C.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _count(lib, torch, labels, gold, m, ng, form, table):
    rc = lib.rae_cluster_count(_p(labels), _p(gold), int(labels.shape[0]), m, ng, form, _p(table),
                               _stream(torch, table.device))
    assert rc == 0, lib.rae_last_error()


def _b3(lib, torch, table, sizes, na, m, ng, out, sizes_out):
    rc = lib.rae_b3_metrics(_p(table), _p(sizes), int(na), m, ng, _p(out), _p(sizes_out),
                            _stream(torch, table.device))
    assert rc == 0, lib.rae_last_error()


def _random_rows(g, n, m, ng):
    """Labels with a few out-of-range ids (-1, m), gold ids half unlabelled (-1) with a few
    out-of-range ones (-2, n_gold)."""
    lab = g.randint(0, m, n).astype(np.int64)
    u = g.rand(n)
    lab[u < 0.02] = -1
    lab[u > 0.98] = m
    gold = g.randint(0, max(ng, 1), n).astype(np.int32)
    v = g.rand(n)
    gold[v < 0.5] = -1
    gold[(v >= 0.5) & (v < 0.53)] = -2
    gold[(v >= 0.53) & (v < 0.56)] = ng
    if ng == 0:
        gold[v >= 0.56] = 0           # == n_gold: out of range too
    return lab, gold


def _forms(_lib, m, ng):
    fits = m * (ng + 1) <= _lib.RAE_CCOUNT_LDS_CELLS
    forms = [_lib.RAE_CCOUNT_GLOBAL, _lib.RAE_CCOUNT_AUTO] + ([_lib.RAE_CCOUNT_LDS] if fits else [])
    return fits, forms


# ---------------------------------------------------------------------------- 1. the table
def test_shapes_cross_the_lds_budget():
    from rae import _lib
    fits = [m * (ng + 1) <= _lib.RAE_CCOUNT_LDS_CELLS for m, ng in SHAPES]
    assert fits == [True, True, True, True, False, False]
    assert SIZES[-1] > 256 * 4 * 2          # more than one pass of a thread's loop


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}-g{s[1]}")
def test_table_is_exact(built_lib, cuda_dev, shape):
    """Every size, pointer offset and form gives contingency_table's counts bit for bit.  Above
    the LDS budget AUTO can only be the global form (an explicit LDS request is refused); within
    it AUTO is documented to be the LDS form, and LDS and GLOBAL are both run explicitly."""
    import torch
    from rae import _lib
    from rae.evaluation import contingency_table
    lib, (m, ng) = built_lib, shape
    fits, forms = _forms(_lib, m, ng)
    g = np.random.RandomState(1000 * m + ng)
    nmax = max(SIZES) + 3
    lab, gold = _random_rows(g, nmax, m, ng)
    lab_d = torch.as_tensor(lab, device=cuda_dev)
    gold_d = torch.as_tensor(gold, device=cuda_dev)
    assert lab_d.data_ptr() % 16 == 0 and gold_d.data_ptr() % 16 == 0
    tb = torch.empty(m * (ng + 1), dtype=torch.int64, device=cuda_dev)
    if not fits:
        rc = lib.rae_cluster_count(_p(lab_d), _p(gold_d), 10, m, ng, _lib.RAE_CCOUNT_LDS, _p(tb),
                                   _stream(torch, cuda_dev))
        assert rc == -1 and b"LDS" in lib.rae_last_error()
    bad = []
    for n in SIZES:
        for off in (0, 1, 3):
            want = torch.as_tensor(contingency_table(lab[off:off + n], _gi(gold[off:off + n], ng), m)
                                   .reshape(-1), device=cuda_dev)
            for form in forms:
                tb.fill_(-7)                                  # dirty: the call zeroes it
                _count(lib, torch, lab_d[off:off + n], gold_d[off:off + n], m, ng, form, tb)
                if not torch.equal(tb, want):
                    bad.append((n, off, form, int((tb != want).sum())))
    # labels and gold offset differently: no head aligns both (gold ids read as dwords), after a
    # head of 1 (1/2) or of none (0/1); and a common head of 2 (0/2)
    n = 4097
    for lo, go in ((1, 2), (0, 1), (0, 2)):
        want = torch.as_tensor(contingency_table(lab[lo:lo + n], _gi(gold[go:go + n], ng), m)
                               .reshape(-1), device=cuda_dev)
        for form in forms:
            _count(lib, torch, lab_d[lo:lo + n], gold_d[go:go + n], m, ng, form, tb)
            if not torch.equal(tb, want):
                bad.append((n, f"{lo}/{go}", form, int((tb != want).sum())))
    assert not bad, bad


def test_table_past_the_grid_cap(built_lib, cuda_dev):
    """More rows than the capped LDS grid covers at four quads per thread."""
    import torch
    from rae import _lib
    from rae.evaluation import contingency_table
    m, ng, n = 100, 7, GRID_CAP_ROWS_LDS + 2851
    lab, gold = _random_rows(np.random.RandomState(5), n + 1, m, ng)
    lab_d = torch.as_tensor(lab, device=cuda_dev)[1:]
    gold_d = torch.as_tensor(gold, device=cuda_dev)[1:]
    want = torch.as_tensor(contingency_table(lab[1:], _gi(gold[1:], ng), m).reshape(-1),
                           device=cuda_dev)
    tb = torch.empty(m * (ng + 1), dtype=torch.int64, device=cuda_dev)
    for form in (_lib.RAE_CCOUNT_LDS, _lib.RAE_CCOUNT_GLOBAL, _lib.RAE_CCOUNT_AUTO):
        _count(built_lib, torch, lab_d, gold_d, m, ng, form, tb)
        assert torch.equal(tb, want), form


# --------------------------------------------------------------------------------- 2. skew
@pytest.mark.parametrize("spread", [False, True], ids=["one-cell", "one-cluster"])
def test_skewed_rows(built_lib, cuda_dev, spread):
    import torch
    from rae import _lib
    from rae.evaluation import contingency_table
    m, ng, n = 100, 41, 4096
    lab = np.full(n, 37, dtype=np.int64)
    gold = (np.arange(n) % (ng + 1) - 1).astype(np.int32) if spread else np.full(n, -1, np.int32)
    want = torch.as_tensor(contingency_table(lab, _gi(gold, ng), m).reshape(-1), device=cuda_dev)
    assert int(want.max()) == (n if not spread else -(-n // (ng + 1)))
    lab_d, gold_d = torch.as_tensor(lab, device=cuda_dev), torch.as_tensor(gold, device=cuda_dev)
    tb = torch.empty(m * (ng + 1), dtype=torch.int64, device=cuda_dev)
    for form in (_lib.RAE_CCOUNT_LDS, _lib.RAE_CCOUNT_GLOBAL):
        _count(built_lib, torch, lab_d, gold_d, m, ng, form, tb)
        assert torch.equal(tb, want), form


# --------------------------------------------------------------------------- 3. accumulate
@pytest.mark.parametrize("shape", [(100, 41), (512, 127)], ids=lambda s: f"m{s[0]}-g{s[1]}")
def test_accumulate(built_lib, cuda_dev, shape):
    import torch
    from rae import _lib
    lib, (m, ng) = built_lib, shape
    n, h = 5001, 2499
    lab, gold = _random_rows(np.random.RandomState(8), n, m, ng)
    lab_d, gold_d = torch.as_tensor(lab, device=cuda_dev), torch.as_tensor(gold, device=cuda_dev)
    ACC = _lib.RAE_CCOUNT_ACCUMULATE
    for form in _forms(_lib, m, ng)[1]:
        whole = torch.zeros(m * (ng + 1), dtype=torch.int64, device=cuda_dev)
        _count(lib, torch, lab_d, gold_d, m, ng, form, whole)
        parts = torch.full_like(whole, 99)                     # dirty: the first call zeroes
        _count(lib, torch, lab_d[:h], gold_d[:h], m, ng, form, parts)
        _count(lib, torch, lab_d[h:], gold_d[h:], m, ng, form | ACC, parts)
        assert torch.equal(parts, whole), form
        # accumulating with no rows leaves the table, counting no rows zeroes it
        _count(lib, torch, lab_d[:0], gold_d[:0], m, ng, form | ACC, parts)
        assert torch.equal(parts, whole), form
        _count(lib, torch, lab_d[:0], gold_d[:0], m, ng, form, parts)
        assert int(parts.abs().sum()) == 0, form


# ------------------------------------------------------------------------------ 4. metrics
def _metrics(lib, torch, dev, tb, sizes, na, m, ng, with_sizes=True):
    out = torch.full((4,), -1.0, dtype=torch.float64, device=dev)
    so = torch.full((m,), -1, dtype=torch.int64, device=dev) if with_sizes else None
    sz = torch.as_tensor(np.asarray(sizes, dtype=np.int64), device=dev) if ng else None
    _b3(lib, torch, tb, sz, na, m, ng, out, so)
    return out.cpu().numpy(), (so.cpu().numpy() if with_sizes else None)


# T = m * n_gold <= 4096 terms per sum: |device - host| <= T 2^-52 relative < 1e-12
@pytest.mark.parametrize("shape", [(1, 0), (3, 1), (100, 40), (64, 64), (512, 8), (7, 130)],
                         ids=lambda s: f"m{s[0]}-g{s[1]}")
def test_metrics_match_the_oracle(built_lib, cuda_dev, shape):
    import torch
    from rae import _lib
    from rae.evaluation import b3_from_table
    lib, (m, ng) = built_lib, shape
    assert m * ng <= 4096
    g = np.random.RandomState(77 + m)
    n = 30011
    lab, gold = _random_rows(g, n, m, ng)
    lab[lab == min(2, m - 1)] = -1 if m > 1 else 0            # an empty cluster (m > 1)
    lab_d, gold_d = torch.as_tensor(lab, device=cuda_dev), torch.as_tensor(gold, device=cuda_dev)
    # the whole gold standard is larger than the labelled rows' share of it (dropped tail)
    sizes = np.bincount(gold[(gold >= 0) & (gold < ng)], minlength=ng)[:ng] + g.randint(0, 5, ng)
    na = int(sizes.sum())
    tables, res = [], []
    for form in (_lib.RAE_CCOUNT_LDS, _lib.RAE_CCOUNT_GLOBAL):
        tb = torch.empty(m * (ng + 1), dtype=torch.int64, device=cuda_dev)
        _count(lib, torch, lab_d, gold_d, m, ng, form, tb)
        tables.append(tb)
        for _ in range(2):
            res.append(_metrics(lib, torch, cuda_dev, tb, sizes, na, m, ng))
    assert torch.equal(tables[0], tables[1])
    first = res[0][0]
    for met, so in res[1:]:                      # run to run and form to form: bitwise
        assert met.tobytes() == first.tobytes()
        assert np.array_equal(so, res[0][1])
    host = tables[0].cpu().numpy().reshape(m, ng + 1)
    f1, pre, rec = b3_from_table(host, sizes, na)
    print("device", first.tolist(), "host", (f1, pre, rec))
    assert first[0] == pytest.approx(f1, rel=1e-12)
    assert first[1] == pytest.approx(pre, rel=1e-12)
    assert first[2] == pytest.approx(rec, rel=1e-12)
    assert first[3] == float(host.sum())
    assert np.array_equal(res[0][1], host.sum(axis=1)) and res[0][1].sum() == first[3]
    # sizes_out == NULL: same metrics
    met, so = _metrics(lib, torch, cuda_dev, tables[0], sizes, na, m, ng, with_sizes=False)
    assert so is None and met.tobytes() == first.tobytes()


def test_metrics_edge_cases(built_lib, cuda_dev):
    import torch
    from rae.evaluation import b3_from_table
    lib = built_lib
    #                 gold0 gold1 gold2 unlabelled
    host = np.array([[3, 1, 0, 2],
                     [0, 0, 0, 5],          # a cluster with only unlabelled members
                     [1, 4, 0, 0],
                     [0, 0, 0, 0]], dtype=np.int64)
    tb = torch.as_tensor(host.reshape(-1), device=cuda_dev)
    m, ng = 4, 3
    sizes = [6, 5, 0]                       # gold class 2 has size 0
    met, so = _metrics(lib, torch, cuda_dev, tb, sizes, 11, m, ng)
    pre = (9 / 4 + 1 / 4 + 1 / 5 + 16 / 5) / 11
    rec = (9 / 6 + 1 / 5 + 1 / 6 + 16 / 5) / 11
    assert met[1] == pytest.approx(pre, rel=1e-12) and met[2] == pytest.approx(rec, rel=1e-12)
    assert met[0] == pytest.approx(2 * pre * rec / (pre + rec), rel=1e-12)
    assert met[:3].tolist() == pytest.approx(list(b3_from_table(host, sizes, 11)), rel=1e-12)
    assert met[3] == 16.0 and so.tolist() == [6, 5, 5, 0] and so.sum() == met[3]
    # a size-0 class whose column is NOT empty still adds nothing
    met0, _ = _metrics(lib, torch, cuda_dev, tb, [6, 0, 0], 11, m, ng)
    assert met0[2] == pytest.approx((9 / 6 + 1 / 6) / 11, rel=1e-12)
    # |A| == 0 -> (0, 0, 0), the element count and the sizes are still reported
    metz, soz = _metrics(lib, torch, cuda_dev, tb, sizes, 0, m, ng)
    assert metz.tolist() == [0.0, 0.0, 0.0, 16.0] and soz.tolist() == [6, 5, 5, 0]
    # nothing labelled in any cluster: precision = recall = 0 and f1 = 0 (not 0/0)
    only = torch.as_tensor(np.array([[0, 0, 0, 4], [0, 0, 0, 1]], dtype=np.int64).reshape(-1),
                           device=cuda_dev)
    metn, _ = _metrics(lib, torch, cuda_dev, only, sizes, 11, 2, ng)
    assert metn.tolist() == [0.0, 0.0, 0.0, 5.0]


# ------------------------------------------------------------------------- engine fixtures
def _inducer(data, gold, dev, m=10, r=16, s=4, l=100, epochs=2, seed=2, freq=False, **kw):
    from rae.inducer import ReconstructInducer
    return ReconstructInducer(data, gold, np.random.RandomState(seed), epochs, 0.1, l, r, m, s,
                              0.0, 0.0, "adagrad", "cl", "sp", False, True, freq, 1.0,
                              device=dev, graph_chunk=8, **kw)


@pytest.fixture(scope="module")
def syn():
    from rae.data import synthetic_dataset
    return synthetic_dataset(20000, 4000, 10, seed=7, gold_fraction=0.05)


def _three_splits(N=850, d=300, ntrue=4, seed=31, cut=(250, 560)):
    """train 250 rows (5 batches of 50), valid 310 and test 290 rows (tails of 10 / 40 rows
    dropped by the batch loop), a gold standard on valid and test."""
    from rae.data import DatasetManager, DatasetSplit, synthetic_dataset
    full, gold = synthetic_dataset(N, d, ntrue, seed=seed, gold_fraction=0.4)
    tr = full.split["train"]
    n = full.get_arg_voc_size()
    a, b = cut
    mk = lambda lo, hi: DatasetSplit(tr.args1[lo:hi], tr.args2[lo:hi], tr.xFeats[lo:hi])
    data = DatasetManager.from_arrays(tr.xFeats[:a], tr.args1[:a], tr.args2[:a], n_entities=n,
                                      n_features=d, valid=mk(a, b), test=mk(b, N))
    g = gold["train"]
    gs = {"train": {}, "valid": {i - a: v for i, v in g.items() if a <= i < b},
          "test": {i - b: v for i, v in g.items() if i >= b}}
    return data, gs


def _record_scores(ind):
    """The (split, (f1, pre, rec)) of every _evaluate call learn() makes."""
    seen, orig = [], ind._evaluate

    def wrapped(split, verbose=True):
        res = orig(split, verbose=verbose)
        seen.append((split, res))
        return res
    ind._evaluate = wrapped
    return seen


def _same_params(a, b):
    import torch
    pa, pb = a.modelFunc.named_params(), b.modelFunc.named_params()
    return all(torch.equal(pa[k], pb[k]) for k in pa)


# -------------------------------------------------------------------------------- 5. graph
def test_label_count_metrics_graph(built_lib, cuda_dev, syn):
    """label -> count -> metrics captured into one HIP graph: the replay gives the eager
    table and metrics bit for bit, and again after W changed."""
    import torch
    from rae.evaluation import GoldIndex
    data, gold = syn
    ind = _inducer(data, gold, cuda_dev)
    ind.compile_function()
    eng = ind.engine
    gi = GoldIndex(gold["train"], eng.split.N)
    cells = eng.m * (gi.n_gold + 1)
    n = 4999

    def snapshot():
        torch.cuda.synchronize()
        return eng._cl_table[:cells].clone(), eng._cl_out.clone()

    eng.queue_cluster_metrics(eng.split, gi, 3, n)          # eager (and the one allocation)
    eager = snapshot()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(cuda_dev)
    s.wait_stream(torch.cuda.current_stream(cuda_dev))
    with torch.cuda.graph(g, stream=s):
        eng.queue_cluster_metrics(eng.split, gi, 3, n)
    torch.cuda.current_stream(cuda_dev).wait_stream(s)
    eng._cl_table.fill_(5)
    eng._cl_out.fill_(5)
    g.replay()
    got = snapshot()
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
    assert int(eager[0].sum()) == n
    # new weights: the replay follows them
    W = ind.modelFunc.params[0]
    gen = torch.Generator(device="cpu").manual_seed(3)
    W.copy_(torch.randn(W.shape, generator=gen).to(cuda_dev))
    eng.queue_cluster_metrics(eng.split, gi, 3, n)
    eager2 = snapshot()
    assert not torch.equal(eager2[0], eager[0])
    eng._cl_table.fill_(5)
    eng._cl_out.fill_(5)
    g.replay()
    got2 = snapshot()
    assert torch.equal(got2[0], eager2[0]) and torch.equal(got2[1], eager2[1])
    eng.close()


# ------------------------------------------------------------------------------- 6. engine
def test_engine_cluster_metrics(built_lib, cuda_dev, syn):
    import torch
    from rae.evaluation import GoldIndex, b3_from_table, contingency_table
    data, gold = syn
    ind = _inducer(data, gold, cuda_dev, epochs=1)
    ind.learn(verbose=False)                                   # trained weights: many clusters
    eng, sp_ = ind.engine, ind.engine.split
    gi = GoldIndex(gold["train"], sp_.N)
    lab, _ = eng.label(sp_, 0, sp_.N, probs=False)
    lab = lab.cpu().numpy()
    assert len(set(lab.tolist())) > 1

    def check(res, r0, n):
        sub = types.SimpleNamespace(ids=gi.ids[r0:r0 + n], n_gold=gi.n_gold, n_rows=n)
        want = contingency_table(lab[r0:r0 + n], sub, eng.m)
        assert np.array_equal(res.table, want)
        assert res.n_elements == n and np.array_equal(res.sizes, want.sum(axis=1))
        assert (res.f1, res.precision, res.recall) == pytest.approx(
            b3_from_table(want, gi.sizes, gi.n_assessable), rel=1e-12)

    whole = eng.cluster_metrics(sp_, gi, table=True)
    check(whole, 0, sp_.N)
    assert eng.cluster_metrics(sp_, gi).table is None
    for r0, n in ((0, 19900), (1, 777), (12345, 4097), (19999, 1), (500, 0)):
        check(eng.cluster_metrics(sp_, gi, r0, n, table=True), r0, n)
    for form in ("lds", "global"):
        res = eng.cluster_metrics(sp_, gi, table=True, form=form)
        assert np.array_equal(res.table, whole.table) and res[:4] == whole[:4]
    with pytest.raises(IndexError):
        eng.cluster_metrics(sp_, gi, 10, sp_.N)
    with pytest.raises(ValueError):
        eng.cluster_metrics(sp_, gi, form="shared")
    # behind an evaluate() and behind a queued training step on the same stream
    eng.evaluate(sp_, 0, 1000)
    again = eng.cluster_metrics(sp_, gi, table=True)
    assert np.array_equal(again.table, whole.table) and again[:4] == whole[:4]
    ind.engine.sample_epoch_negatives(ind.negativeSampler, "device", 0, 1)
    eng.run(0, 1, graph=False)
    after = eng.cluster_metrics(sp_, gi, table=True)
    lab2, _ = eng.label(sp_, 0, sp_.N, probs=False)
    assert np.array_equal(after.table, contingency_table(lab2.cpu().numpy(), gi, eng.m))
    # the gold arrays are uploaded once per (split, gold index)
    assert eng._gold_dev(sp_, gi)[0] is eng._gold_dev(sp_, gi)[0]
    eng.close()


# --------------------------------------------------------------------------- 7. end to end
def test_learn_host_and_device_agree(built_lib, cuda_dev, syn):
    """synthetic:20000, K = 10, two epochs from one seed, scored on the host and on the
    device: the parameters are bitwise equal (the evaluation touches no training state), the
    per-epoch triples agree to rel 1e-12 and get_clusters_size is equal."""
    import torch
    data, gold = syn
    runs = {}
    for mode in ("host", "device"):
        ind = _inducer(data, gold, cuda_dev, cluster_eval=mode)
        seen = _record_scores(ind)
        ind.learn(verbose=False)
        torch.cuda.synchronize()
        runs[mode] = (ind, seen, ind.get_clusters_size("train"))
    (hi, hs, hc), (di, ds, dc) = runs["host"], runs["device"]
    assert _same_params(hi, di)
    assert hi.train_errors == di.train_errors
    assert [s for s, _ in hs] == [s for s, _ in ds] == ["train", "train"]
    for (_, a), (_, b) in zip(hs, ds):
        print("host", a, "device", b)
        assert a[1] > 0 and a[2] > 0
        assert b == pytest.approx(a, rel=1e-12)
    assert isinstance(dc, Counter) and dc == hc and sum(dc.values()) == 20000
    assert all(v > 0 for v in dc.values())
    assert di.cluster["train"] is None and hi.cluster["train"] is not None
    # the sets are still there on demand
    sets = di.get_clusters_sets("train")
    assert {c: len(v) for c, v in sets.items() if v} == dict(dc)
    hi.engine.close()
    di.engine.close()


def test_frequent_eval_host_and_device_agree(built_lib, cuda_dev, capsys):
    """frequentEval over 5 batches (valid and test scored after every batch, then per epoch)."""
    import torch
    data, gold = _three_splits()
    runs = {}
    for mode in ("host", "device"):
        ind = _inducer(data, gold, cuda_dev, m=6, l=50, epochs=1, freq=True, cluster_eval=mode)
        assert ind.batch_reps["train"] == 5
        seen = _record_scores(ind)
        ind.learn(verbose=True)
        torch.cuda.synchronize()
        runs[mode] = (ind, seen, capsys.readouterr().out)
    (hi, hs, ho), (di, ds, do) = runs["host"], runs["device"]
    assert _same_params(hi, di)
    assert [s for s, _ in hs] == [s for s, _ in ds] == ["valid", "test"] * 6
    for (_, a), (_, b) in zip(hs, ds):
        assert b == pytest.approx(a, rel=1e-12)
    assert any(a[0] > 0 for _, a in hs)
    # the same lines (the epoch duration aside)
    strip = lambda out: [ln for ln in out.splitlines() if not ln.startswith("Epoch duration")]
    assert strip(ho) == strip(do)
    for split in ("valid", "test"):
        assert hi.get_clusters_size(split) == di.get_clusters_size(split)
    hi.engine.close()
    di.engine.close()
