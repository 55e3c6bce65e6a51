"""Cluster exemplars on the GPU (rae_label_stats, rae_cluster_exemplars; TrainEngine.label_stats /
cluster_exemplars / cluster_confidence; ReconstructInducer(print_exemplars=...)) against the numpy
oracles of rae/evaluation.py, and rae_label_stats against rae_label itself.  Every shape is tiny:
what is covered is the kernels' paths (both vector widths, 16 / 32 / 64 lanes per row, one or two
column chunks per lane, the feature seams of the gather; every view offset, several strips, 4 / 2 /
1 waves per workgroup, the 128 KiB list form), not their throughput."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from _profile_sample import sample_data
from rae.evaluation import cluster_exemplars, format_cluster_exemplars, label_stats

pytestmark = pytest.mark.gpu


def _dev(torch, a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _eq(a, b):
    """Equal with ==, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# --------------------------------------------------------------------------- 1. label stats
class Split:
    """A CSR matrix in HBM (values None: binary, the kernel's values == NULL path)."""

    def __init__(self, torch, dev, X, binary=False):
        X = sp.csr_matrix(X)
        self.X, self.N = X, X.shape[0]
        self.indptr = _dev(torch, X.indptr.astype(np.int32), dev)
        self.indices = _dev(torch, np.concatenate([X.indices, [0]]).astype(np.int32), dev)
        self.values = None if binary else \
            _dev(torch, np.concatenate([X.data, [0]]).astype(np.float32), dev)


def _stats(lib, torch, dev, s, W, Wb, row0=0, nrows=None, margin=True, pmax=True):
    """rae_label_stats through the C ABI: (labels, margin, pmax) as numpy arrays (None if not asked)."""
    from rae import _lib
    nrows = s.N - row0 if nrows is None else nrows
    m = W.shape[1]
    lab = torch.full((max(nrows, 1),), -7, dtype=torch.int64, device=dev)
    mar = torch.full((max(nrows, 1),), 77.0, dtype=torch.float32, device=dev) if margin else None
    pm = torch.full((max(nrows, 1),), 77.0, dtype=torch.float32, device=dev) if pmax else None
    _lib.check(lib.rae_label_stats(
        _lib.ptr(s.indptr), _lib.ptr(s.indices), _lib.ptr(s.values), _lib.ptr(W), _lib.ptr(Wb), m,
        row0, nrows, _lib.ptr(lab), _lib.ptr(mar), _lib.ptr(pm), None), "rae_label_stats")
    torch.cuda.synchronize()
    out = [lab.cpu().numpy()[:nrows]]
    out += [None if t is None else t.cpu().numpy()[:nrows] for t in (mar, pm)]
    return tuple(out)


def _label(lib, torch, dev, s, W, Wb):
    from rae import _lib
    m = W.shape[1]
    lab = torch.empty(s.N, dtype=torch.int64, device=dev)
    pr = torch.empty((s.N, m), dtype=torch.float32, device=dev)
    _lib.check(lib.rae_label(_lib.ptr(s.indptr), _lib.ptr(s.indices), _lib.ptr(s.values),
                             _lib.ptr(W), _lib.ptr(Wb), m, 0, s.N, _lib.ptr(lab), _lib.ptr(pr),
                             None), "rae_label")
    torch.cuda.synchronize()
    return lab.cpu().numpy(), pr.cpu().numpy()


def _ragged(g, d, lengths, values):
    """Row i holds lengths[i] distinct features with values drawn by values(n)."""
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([g.choice(d, n, replace=False) for n in lengths] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((values(int(indptr[-1])).astype(np.float32), idx.astype(np.int32),
                          indptr), shape=(len(lengths), d))


STATS_M = (1, 2, 3, 4, 7, 12, 64, 65, 100, 128, 132, 256, 260, 512)


@pytest.mark.parametrize("m", STATS_M)
def test_label_stats_exact_on_dyadic_data(built_lib, cuda_dev, m):
    """W, Wb integers in [-64, 64] / 8, values in {1, 2, 3} (or binary): every fp32 sum is exact in
    any order (|S| * 8 <= 130 * 3 * 64 + 64 < 2^24), so labels and margin equal the float32 oracle
    with ==.  Rows of every length 0 ... 130: the 17 / 33 feature seam of 16 / 32 lanes per row and
    the 64 / 65 chunk seam; an empty row's margin is Wb's."""
    import torch
    g = np.random.RandomState(100 + m)
    d = 200
    W = (g.randint(-64, 65, (d, m)) / 8.0).astype(np.float32)
    Wb = (g.randint(-64, 65, m) / 8.0).astype(np.float32)
    Wd, Wbd = _dev(torch, W, cuda_dev), _dev(torch, Wb, cuda_dev)
    lengths = np.arange(131)
    for binary in (False, True):
        X = _ragged(g, d, lengths, (lambda n: np.ones(n)) if binary else
                    (lambda n: g.randint(1, 4, n)))
        s = Split(torch, cuda_dev, X, binary)
        lab, mar, pm = _stats(built_lib, torch, cuda_dev, s, Wd, Wbd)
        wl, wm, wp = label_stats(X, W, Wb)
        assert np.array_equal(lab, wl), (m, binary)
        assert _eq(mar, wm), (m, binary, mar[:5], wm[:5])
        if m == 1:
            assert np.all(np.isposinf(mar)) and np.array_equal(pm, np.ones(131, np.float32))
        else:
            assert np.all(mar >= 0)
            # two sums of m positive terms in another order: gamma_m each, and expf's few ulp
            np.testing.assert_allclose(pm, wp, rtol=2 * (m + 8) * 2.0 ** -24)
        # the optional outputs change nothing
        only = _stats(built_lib, torch, cuda_dev, s, Wd, Wbd, margin=False, pmax=False)
        assert np.array_equal(only[0], lab) and only[1] is None and only[2] is None


def _positions(m):
    return sorted(p for p in {0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 260, m - 2, m - 1}
                  if 0 <= p < m)


@pytest.mark.parametrize("m", (2, 7, 65, 100, 132, 512))
def test_label_stats_best_and_second_in_every_relative_position(built_lib, cuda_dev, m):
    """One stored feature per row, so S is a row of W: best (5) and second (3) at every ordered pair
    of positions -- the same float4, the same lane's other element or other column chunk (col and
    col + 64), different lanes, best last and second first -- over a distinct descending
    background; an exact two-way tie (margin 0, the first column); all columns equal."""
    import torch
    pos = _positions(m)
    rows, want = [], []
    base = (-10.0 - 0.25 * np.arange(m)).astype(np.float32)
    for pb in pos:
        for ps in pos:
            if pb == ps:
                continue
            r = base.copy()
            r[pb], r[ps] = 5.0, 3.0
            rows.append(r)
            want.append((pb, 2.0))
            r = base.copy()
            r[pb] = r[ps] = 5.0                            # a two-way tie
            rows.append(r)
            want.append((min(pb, ps), 0.0))
    rows.append(np.full(m, 1.5, np.float32))               # all equal
    want.append((0, 0.0))
    W = np.stack(rows)
    N = W.shape[0]
    s = Split(torch, cuda_dev, sp.identity(N, dtype=np.float32, format="csr"))
    Wb = np.zeros(m, np.float32)
    lab, mar, pm = _stats(built_lib, torch, cuda_dev, s, _dev(torch, W, cuda_dev),
                          _dev(torch, Wb, cuda_dev))
    assert lab.tolist() == [w[0] for w in want]
    assert mar.tolist() == [w[1] for w in want]
    wl, wm, _ = label_stats(s.X, W, Wb)
    assert np.array_equal(lab, wl) and _eq(mar, wm)


@pytest.mark.parametrize("m", (3, 7, 100, 512))
def test_label_stats_nan_and_infinity(built_lib, cuda_dev, m):
    """A NaN in one column (the label, NaN counting as the maximum; margin NaN), a NaN in two (the
    first is the label), +inf twice (inf - inf: NaN), one +inf (margin +inf), -inf everywhere.
    One stored feature of value 2 per row, so S is twice a row of W."""
    import torch
    pos = _positions(m)
    base = (0.5 * np.arange(m)).astype(np.float32)
    rows, labels, kinds = [], [], []
    for a in pos:
        r = base.copy(); r[a] = np.nan
        rows.append(r); labels.append(a); kinds.append("nan")
        r = base.copy(); r[a] = np.inf
        rows.append(r); labels.append(a); kinds.append("inf")
        for b in pos:
            if a < b:
                r = base.copy(); r[a] = r[b] = np.nan
                rows.append(r); labels.append(a); kinds.append("nan")
                r = base.copy(); r[a] = r[b] = np.inf
                rows.append(r); labels.append(a); kinds.append("nan")
                r = base.copy(); r[a], r[b] = np.nan, np.inf
                rows.append(r); labels.append(a); kinds.append("nan")
    rows.append(np.full(m, -np.inf, np.float32)); labels.append(0); kinds.append("nan")
    # S = 2 W: an infinite logit comes from an overflowing product (an infinite WEIGHT would meet
    # the gather's zero-valued padding slots, 0 * inf, in rae_label as well); a NaN weight is a NaN
    S = np.stack(rows)
    with np.errstate(invalid="ignore"):
        W = np.where(np.isinf(S), np.sign(S) * np.float32(3e38), S / 2).astype(np.float32)
    s = Split(torch, cuda_dev, 2.0 * sp.identity(W.shape[0], dtype=np.float32, format="csr"))
    Wb = np.zeros(m, np.float32)
    lab, mar, pm = _stats(built_lib, torch, cuda_dev, s, _dev(torch, W, cuda_dev),
                          _dev(torch, Wb, cuda_dev))
    assert lab.tolist() == labels
    assert [("nan" if np.isnan(x) else "inf" if np.isposinf(x) else x) for x in mar] == kinds
    wl, wm, _ = label_stats(s.X, W, Wb)
    assert np.array_equal(lab, wl) and _eq(mar, wm)


def _normal_problem(m, seed):
    g = np.random.RandomState(seed)
    d = 300
    X = _ragged(g, d, np.arange(131), lambda n: g.standard_normal(n))
    return X, g.standard_normal((d, m)).astype(np.float32), g.standard_normal(m).astype(np.float32)


@pytest.mark.parametrize("m", (100, 30, 7))
def test_label_stats_against_rae_label_on_float_data(built_lib, cuda_dev, m):
    """Standard-normal values, W and Wb: labels bitwise rae_label's, pmax bitwise probs[i, label],
    and |margin - margin64| <= 2 max_k gamma_{nf+4} (sum_j |v_j W[f_j, k]| + |Wb_k|), gamma_n =
    n u / (1 - n u), u = 2^-24: best minus second-best is 2-Lipschitz in the logits' largest error,
    whatever the labels, so every row is held to it."""
    import torch
    X, W, Wb = _normal_problem(m, 7 + m)
    s = Split(torch, cuda_dev, X)
    Wd, Wbd = _dev(torch, W, cuda_dev), _dev(torch, Wb, cuda_dev)
    lab, mar, pm = _stats(built_lib, torch, cuda_dev, s, Wd, Wbd)
    rl, rp = _label(built_lib, torch, cuda_dev, s, Wd, Wbd)
    assert np.array_equal(lab, rl)
    assert np.array_equal(_bits(pm), _bits(rp[np.arange(s.N), rl]))
    _, m64, _ = label_stats(X, W, Wb, dtype=np.float64)
    nf = np.diff(X.indptr).astype(np.float64)
    u = 2.0 ** -24
    gamma = (nf + 4) * u / (1 - (nf + 4) * u)
    mag = (abs(X).astype(np.float64) @ np.abs(W).astype(np.float64) +
           np.abs(Wb).astype(np.float64)[None, :]).max(axis=1)
    err = np.abs(mar.astype(np.float64) - m64)
    bound = 2 * gamma * np.asarray(mag).reshape(-1)
    print("margin error / bound, worst row:", float((err / bound).max()))
    assert np.all(err <= bound), (err.max(), (err / bound).max())
    assert np.all(mar >= 0)


def test_label_stats_rows_are_independent(built_lib, cuda_dev):
    """All three outputs bitwise equal over a sub-range, a shifted row0, a row permutation of the
    split and a repeated call."""
    import torch
    m = 100
    X, W, Wb = _normal_problem(m, 11)
    s = Split(torch, cuda_dev, X)
    Wd, Wbd = _dev(torch, W, cuda_dev), _dev(torch, Wb, cuda_dev)
    full = _stats(built_lib, torch, cuda_dev, s, Wd, Wbd)
    same = lambda a, b: all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                           y.view(np.uint32) if y.dtype == np.float32 else y)
                            for x, y in zip(a, b))
    assert same(full, _stats(built_lib, torch, cuda_dev, s, Wd, Wbd))
    for row0, nrows in ((17, 50), (5, s.N - 5), (130, 1), (64, 0)):
        part = _stats(built_lib, torch, cuda_dev, s, Wd, Wbd, row0, nrows)
        assert same(part, tuple(x[row0:row0 + nrows] for x in full)), (row0, nrows)
    perm = np.random.RandomState(1).permutation(s.N)
    sp_ = Split(torch, cuda_dev, X[perm])
    assert same(_stats(built_lib, torch, cuda_dev, sp_, Wd, Wbd), tuple(x[perm] for x in full))


# --------------------------------------------------------------------------- 2. cluster exemplars
def _exemplars(lib, torch, dev, labels, scores, m, top, largest=True, loff=0, soff=0,
               want_scores=True):
    """rae_cluster_exemplars through the C ABI on views that start loff / soff elements into their
    buffers; the workspace and the outputs start out as garbage."""
    from rae import _lib
    n = len(labels)
    lb = torch.full((n + 4,), 3, dtype=torch.int64, device=dev)
    sb = torch.full((n + 4,), 1e30, dtype=torch.float32, device=dev)
    if n:
        lb[loff:loff + n] = _dev(torch, np.asarray(labels, np.int64), dev)
        sb[soff:soff + n] = _dev(torch, np.asarray(scores, np.float32), dev)
    a = _lib.RaeExemplarArgs()
    a.labels, a.scores, a.nrows = lb.data_ptr() + 8 * loff, sb.data_ptr() + 4 * soff, n
    a.relations, a.top, a.largest = m, top, int(largest)
    need = lib.rae_cluster_exemplars_workspace_bytes(C.byref(a))
    assert 0 < need <= 16 << 20
    ws = torch.full((need,), 0x33, dtype=torch.uint8, device=dev)
    ro = torch.full((m, top), -9, dtype=torch.int32, device=dev)
    so = torch.full((m, top), 9.0, dtype=torch.float32, device=dev)
    a.rows_out, a.scores_out = ro.data_ptr(), so.data_ptr() if want_scores else None
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _lib.check(lib.rae_cluster_exemplars(C.byref(a), None), "rae_cluster_exemplars")
    torch.cuda.synchronize()
    return ro.cpu().numpy(), so.cpu().numpy()


def _check(lib, torch, dev, labels, scores, m, top, largest, loff=0, soff=0):
    rows, out = _exemplars(lib, torch, dev, labels, scores, m, top, largest, loff, soff)
    wr, wo = cluster_exemplars(labels, scores, m, top, largest)
    assert np.array_equal(rows, wr), (len(labels), m, top, largest, loff, soff)
    assert np.array_equal(_bits(out), _bits(wo)), (len(labels), m, top, largest, loff, soff)


def _mixed(g, n, m):
    """Labels with -1 and m mixed in; scores from a small set (many duplicates) with NaN, +-inf and
    both zeros among them."""
    lab = g.randint(-1, m + 1, n).astype(np.int64)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 2.5, 1e-30, -3e20, 7.0, 0.125],
                    np.float32)
    return lab, pool[g.randint(0, len(pool), n)]


@pytest.mark.parametrize("n", (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 20011))
def test_exemplars_every_length_and_view_offset(built_lib, cuda_dev, n):
    """Views starting 0 ... 3 elements into their buffers; 20011 rows span several strips."""
    import torch
    from rae import _lib
    g = np.random.RandomState(n)
    m = 7
    lab, sc = _mixed(g, n, m)
    for (loff, soff), top in zip(((0, 0), (1, 1), (2, 3), (3, 2), (0, 1), (1, 0), (2, 2), (3, 3)),
                                 (5, 1, 32, 2, 5, 10, 31, 3)):
        for largest in (True, False):
            _check(built_lib, torch, cuda_dev, lab, sc, m, top, largest, loff, soff)
    assert _lib.cex_strips(20011) == 5


@pytest.mark.parametrize("m", (1, 2, 100, 512))
def test_exemplars_relations_by_top(built_lib, cuda_dev, m):
    """4, 2 and 1 waves per workgroup; 512 x 32 is the 128 KiB list form."""
    import torch
    from rae import _lib
    g = np.random.RandomState(m)
    n = 1025
    lab = g.randint(0, m, n).astype(np.int64)
    sc = g.standard_normal(n).astype(np.float32)
    sc[g.rand(n) < 0.2] = 0.5                                  # duplicates
    for top in (1, 2, 10, 31, 32):
        for largest in (True, False):
            _check(built_lib, torch, cuda_dev, lab, sc, m, top, largest)
    assert [_lib.cex_waves(m, t) for t in (1, 32)] == \
        {1: [4, 4], 2: [4, 4], 100: [4, 2], 512: [4, 1]}[m]


EX_KINDS = ("empty_clusters", "outside_labels", "one_cluster_ascending", "one_cluster_descending",
            "all_equal", "seam_duplicates", "special_values")


@pytest.mark.parametrize("kind", EX_KINDS)
def test_exemplars_label_and_score_cases(built_lib, cuda_dev, kind):
    import torch
    g = np.random.RandomState(EX_KINDS.index(kind))
    n, m = 20011, 5
    lab = g.randint(0, m, n).astype(np.int64)
    sc = g.standard_normal(n).astype(np.float32)
    if kind == "empty_clusters":
        lab = np.where(lab % 2 == 1, 0, lab)                   # clusters 1 and 3 stay empty
    elif kind == "outside_labels":
        lab[g.rand(n) < 0.3] = -1
        lab[g.rand(n) < 0.3] = m
        lab[:3] = (-(1 << 40), 1 << 40, (1 << 32) + 1)         # beyond 32 bits, low word in range
    elif kind == "one_cluster_ascending":                      # largest: every row is admitted
        lab[:], sc = 2, np.arange(n, dtype=np.float32)
    elif kind == "one_cluster_descending":
        lab[:], sc = 2, -np.arange(n, dtype=np.float32)
    elif kind == "all_equal":                                  # row-ascending ties
        sc[:] = 1.25
    elif kind == "seam_duplicates":                            # the same scores in every strip
        sc = (np.arange(n) % 7).astype(np.float32)
    elif kind == "special_values":
        lab, sc = _mixed(g, n, m)
    for top in (1, 10, 32):
        for largest in (True, False):
            _check(built_lib, torch, cuda_dev, lab, sc, m, top, largest)


def test_exemplars_without_scores_out_and_under_permutation(built_lib, cuda_dev):
    import torch
    g = np.random.RandomState(9)
    n, m, top = 5000, 6, 9
    lab = g.randint(0, m, n).astype(np.int64)
    sc = g.permutation(n).astype(np.float32) - 2500.0          # distinct: the order is by score alone
    for largest in (True, False):
        rows, out = _exemplars(built_lib, torch, cuda_dev, lab, sc, m, top, largest)
        r2, o2 = _exemplars(built_lib, torch, cuda_dev, lab, sc, m, top, largest, want_scores=False)
        assert np.array_equal(r2, rows) and np.all(o2 == 9.0)  # scores_out NULL: not written
        perm = g.permutation(n)
        rp, op = _exemplars(built_lib, torch, cuda_dev, lab[perm], sc[perm], m, top, largest)
        assert np.array_equal(np.where(rp >= 0, perm[np.maximum(rp, 0)], -1), rows)
        assert np.array_equal(_bits(op), _bits(out))


# --------------------------------------------------------------------------- 3. end to end
def _inducer(data, gold, dev, m=10, r=10, s=5, l=100, epochs=1, seed=2, **kw):
    from rae.inducer import ReconstructInducer
    return ReconstructInducer(data, gold, np.random.RandomState(seed), epochs, 0.1, l, r, m, s,
                              0.0, 0.0, "adagrad", "cx", "sp", False, True, False, 1.0,
                              device=dev, graph_chunk=8, **kw)


def test_engine_and_inducer_on_the_sample(built_lib, cuda_dev, capsys):
    """After an epoch on the sample: cluster_exemplars by margin and by pmax = the oracle fed with
    label_stats' own outputs, cluster_confidence = the histogram of the downloaded pmax, and the
    lines learn() prints = format_cluster_exemplars of the same tensors."""
    import torch
    from rae.evaluation import KeyIndex, row_keys
    data, gold = sample_data()
    ind = _inducer(data, gold, cuda_dev, print_exemplars=3, print_exemplars_order="both")
    ind.learn(verbose=True)
    torch.cuda.synchronize()
    out = capsys.readouterr().out.splitlines()
    eng, ds = ind.engine, ind._dev_split["train"]
    m = eng.m
    lab_d, mar_d, pm_d = eng.label_stats(ds)
    lab, mar, pm = lab_d.cpu().numpy(), mar_d.cpu().numpy(), pm_d.cpu().numpy()
    rl, rp = eng.label(ds, 0, ds.N)
    assert torch.equal(lab_d, rl) and torch.equal(pm_d, rp[torch.arange(ds.N), rl])
    assert lab_d.dtype == torch.int64 and mar_d.dtype == pm_d.dtype == torch.float32
    for by, sc in (("margin", mar), ("pmax", pm)):
        for largest in (True, False):
            for top in (1, 5, 32):
                res = eng.cluster_exemplars(ds, top=top, by=by, largest=largest)
                wr, wo = cluster_exemplars(lab, sc, m, top, largest)
                assert np.array_equal(res.rows, wr) and np.array_equal(_bits(res.scores), _bits(wo))
    # a sub-range: rows come back as the split's row ids; a caller's scores and labels
    row0, nrows = 37, ds.N - 50
    res = eng.cluster_exemplars(ds, top=4, by="margin", row0=row0, nrows=nrows)
    wr, wo = cluster_exemplars(lab[row0:row0 + nrows], mar[row0:row0 + nrows], m, 4, True)
    assert np.array_equal(res.rows, np.where(wr >= 0, wr + row0, -1))
    assert np.array_equal(_bits(res.scores), _bits(wo))
    mine = torch.arange(ds.N, device=cuda_dev, dtype=torch.float32) % 13
    lab2 = (torch.arange(ds.N, device=cuda_dev) * 7) % m
    res = eng.cluster_exemplars(ds, top=6, by=mine, largest=False, labels=lab2)
    wr, wo = cluster_exemplars(lab2.cpu().numpy(), mine.cpu().numpy(), m, 6, False)
    assert np.array_equal(res.rows, wr) and np.array_equal(_bits(res.scores), _bits(wo))
    with pytest.raises(ValueError):
        eng.cluster_exemplars(ds, top=33)
    with pytest.raises(ValueError):
        eng.cluster_exemplars(ds, by="psi")
    # the confidence histogram
    for bins in (1, 10, 16):
        table = eng.cluster_confidence(ds, bins=bins)
        assert table.dtype == torch.int32 and tuple(table.shape) == (m, bins)
        b = np.minimum((pm * np.float32(bins)).astype(np.int64), bins - 1)
        want = np.zeros((m, bins), np.int32)
        np.add.at(want, (lab[~np.isnan(pm)], b[~np.isnan(pm)]), 1)
        assert np.array_equal(table.cpu().numpy(), want)
        assert int(want.sum()) == ds.N
    # the printed lines: a header and m lines per order, those of the final parameters
    nrows = (ds.N // 100) * 100
    sizes = np.bincount(lab[:nrows], minlength=m)
    ki = KeyIndex.from_lexicon(data.featureLex)
    keys = row_keys(data.split["train"].xFeats, ki.key_of_feature)
    sp_ = data.split["train"]
    want = []
    for largest in (True, False):
        wr, wo = cluster_exemplars(lab[:nrows], mar[:nrows], m, 3, largest)
        want += format_cluster_exemplars(wr, wo, sizes, np.asarray(sp_.args1), np.asarray(sp_.args2),
                                         getattr(data, "id2Arg", None), keys, ki.names)
    lines = [ln for ln in out if ln.startswith("relation ")]
    assert len(lines) == 2 * m and lines == want
    heads = [ln for ln in out if " exemplars, " in ln]
    assert heads == ["train exemplars, most confident by margin",
                     "train exemplars, least confident by margin"]
    assert lines == [ln for ln in ind.cluster_exemplar_lines("train") if ln.startswith("relation ")]
    assert any(" | " in ln for ln in want)
    # the option changes nothing else: the same parameters as a run without it
    ref = _inducer(data, gold, cuda_dev)
    ref.learn(verbose=False)
    pa, pb = ind.modelFunc.named_params(), ref.modelFunc.named_params()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    ref.engine.close()
    eng.close()


def test_smoke(built_lib, cuda_dev):
    import __graft_entry__ as ge
    ge.smoke()
