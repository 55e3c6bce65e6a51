"""Per-cluster profiles on the device (rae_row_keys / rae_cluster_key_count / rae_cluster_topk,
include/rae.h; TrainEngine.cluster_profiles; ReconstructInducer(print_clusters=...)) against the
numpy oracles of rae/evaluation.py, which tests/test_profile_host.py pins to the reference's
print_clusters.  Integer results: exact equality throughout."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from _profile_sample import count_rows, sample_data

pytestmark = pytest.mark.gpu

GUARD = -7


def _p(t, off=0):
    """The tensor's device address (from its storage: an empty view's data_ptr() is 0)."""
    if t is None:
        return None
    return C.c_void_p(t.untyped_storage().data_ptr() + (t.storage_offset() + off) * t.element_size())


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(torch, a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


# --------------------------------------------------------------------------- 1. row keys
def _keyed_csr(seed=4, n=1500, d=3000):
    """A CSR with row lengths cycling {0, 1, 17, 64, 65, 130}, ~10 % of the features keyed,
    ~15 % of the stored values 0, and four crafted rows in every 24: no keyed column; several
    keyed columns; the only keyed column last; a keyed first column whose stored value is 0."""
    g = np.random.RandomState(seed)
    kof = np.where(g.rand(d) < 0.1, g.randint(0, 50, d), -1).astype(np.int32)
    K, U = np.flatnonzero(kof >= 0), np.flatnonzero(kof < 0)
    lengths = [0, 1, 17, 64, 65, 130]
    indptr, idx, val = [0], [], []
    for i in range(n):
        L = lengths[i % 6]
        kind = (i // 6) % 4
        v = np.where(g.rand(L) < 0.15, 0.0, 1.0)
        if L < 2:
            cols = np.sort(g.choice(d, size=L, replace=False))
        elif kind == 0:                                         # no keyed column
            cols = np.sort(g.choice(U, size=L, replace=False))
        elif kind == 1:                                         # several keyed: the first wins
            cols = np.sort(np.concatenate([g.choice(K, size=3, replace=False),
                                           g.choice(U, size=L - 3, replace=False)]))
            v[:] = 1.0
        elif kind == 2:                                         # the only keyed column is last
            last = K[K > d // 2][g.randint(0, (K > d // 2).sum())]
            cols = np.append(np.sort(g.choice(U[U < last], size=L - 1, replace=False)), last)
            v[-1] = 1.0
        else:                                                   # keyed first column, stored 0
            first = K[g.randint(0, 20)]
            rest = np.concatenate([K[K > first][-2:], U[U > first]])
            cols = np.append(first, np.sort(g.choice(rest, size=L - 1, replace=False)))
            v[0] = 0.0
        idx.extend(int(c) for c in cols)
        val.extend(v.tolist())
        indptr.append(len(idx))
    X = sp.csr_matrix((np.array(val, np.float32), np.array(idx, np.int32),
                       np.array(indptr, np.int32)), shape=(n, d))
    return X, kof


def _row_keys(lib, torch, dev, X, kof, row0, nrows, values=True, n_features=None):
    ip, ix = _dev(torch, X.indptr.astype(np.int32), dev), _dev(torch, X.indices.astype(np.int32), dev)
    vv = _dev(torch, X.data.astype(np.float32), dev) if values else None
    kd = _dev(torch, kof, dev)
    out = torch.full((nrows + 8,), GUARD, dtype=torch.int32, device=dev)
    rc = lib.rae_row_keys(_p(ip), _p(ix), _p(vv), _p(kd),
                          kof.shape[0] if n_features is None else n_features, row0, nrows,
                          _p(out, 4), _stream(torch, dev))
    assert rc == 0, lib.rae_last_error()
    host = out.cpu().numpy()
    assert (host[:4] == GUARD).all() and (host[4 + nrows:] == GUARD).all()   # nothing outside
    return host[4:4 + nrows]


def test_row_keys(built_lib, cuda_dev):
    import torch
    from rae.evaluation import row_keys
    X, kof = _keyed_csr()
    n = X.shape[0]
    want = row_keys(X, kof)
    want_nv = row_keys(X, kof, use_values=False)
    # the fixture exercises what it claims to
    nnz = np.diff(X.indptr)
    assert set(nnz.tolist()) == {0, 1, 17, 64, 65, 130}
    keyed = sp.csr_matrix((kof[X.indices] >= 0, X.indices, X.indptr), shape=X.shape)
    nkeyed = np.asarray(keyed.sum(axis=1)).ravel()
    last_keyed = np.array([nnz[i] > 1 and nkeyed[i] == 1 and kof[X.indices[X.indptr[i + 1] - 1]] >= 0
                           for i in range(n)])
    assert ((want == -1) & (nnz > 1)).sum() > 50 and (nkeyed >= 3).sum() > 50
    assert (last_keyed & (want >= 0)).sum() > 50
    assert (want != want_nv).sum() > 50 and ((want != want_nv) & (nnz >= 130)).any()
    assert (want[nnz == 130] >= 0).any() and (want[nnz == 0] == -1).all()
    got = _row_keys(built_lib, torch, cuda_dev, X, kof, 0, n)
    assert np.array_equal(got, want)
    got = _row_keys(built_lib, torch, cuda_dev, X, kof, 0, n, values=False)
    assert np.array_equal(got, want_nv)
    # a row range, and no rows at all
    assert np.array_equal(_row_keys(built_lib, torch, cuda_dev, X, kof, 37, 101), want[37:138])
    assert np.array_equal(_row_keys(built_lib, torch, cuda_dev, X, kof, n - 1, 1), want[n - 1:])
    assert _row_keys(built_lib, torch, cuda_dev, X, kof, 37, 0).shape == (0,)
    # columns at or past n_features carry no key (and key_of_feature is not read there)
    short = kof[:2000]
    want_s = row_keys(X, short)
    assert (want_s != want).any()
    got = _row_keys(built_lib, torch, cuda_dev, X, short, 0, n, n_features=2000)
    assert np.array_equal(got, want_s)
    assert (_row_keys(built_lib, torch, cuda_dev, X, short, 0, n, n_features=0) == -1).all()


# ------------------------------------------------------------------------- 2. the key table
KEY_SHAPES = [(1, 1), (3, 5), (100, 481), (512, 4097), (7, 100003)]
KINDS = ["uniform", "zipf", "one-cell", "one-cluster"]
# (labels offset, keys offset) in elements: both 16-byte aligned; a head of 1; no common head
# (the keys of the middle are read as dwords); a head of 2; no common head with the labels
# aligned (dwords again, no head at all); a head of 3
VIEWS = [(0, 0), (1, 3), (1, 2), (0, 2), (0, 1), (1, 1)]


def _key_count(lib, torch, lab, key, n, m, nk, acc, table):
    rc = lib.rae_cluster_key_count(_p(lab), _p(key), n, m, nk, acc, _p(table),
                                   _stream(torch, table.device))
    assert rc == 0, lib.rae_last_error()


@pytest.mark.parametrize("shape", KEY_SHAPES, ids=lambda s: f"m{s[0]}-k{s[1]}")
def test_key_table_is_exact(built_lib, cuda_dev, shape):
    import torch
    from rae.evaluation import key_table
    lib, (m, nk) = built_lib, shape
    n = 20000
    tb = torch.empty(m * nk + 2, dtype=torch.int32, device=cuda_dev)
    bad = []
    for ki, kind in enumerate(KINDS):
        lab, key = count_rows(np.random.RandomState(100 * ki + m), n + 3, m, nk, kind)
        if kind != "one-cell":
            assert (lab == -1).any() and (lab == m).any() and (key == -1).any() and (key == nk).any()
        lab_d, key_d = _dev(torch, lab, cuda_dev), _dev(torch, key, cuda_dev)
        assert lab_d.data_ptr() % 16 == 0 and key_d.data_ptr() % 16 == 0
        for lo, ko in VIEWS:
            cnt = n - (lo + ko) % 3                       # tails of 0..3 rows
            want = _dev(torch, key_table(lab[lo:lo + cnt], key[ko:ko + cnt], m, nk).reshape(-1),
                        cuda_dev)
            tb.fill_(GUARD)                               # dirty: the call zeroes it
            _key_count(lib, torch, lab_d[lo:], key_d[ko:], cnt, m, nk, 0, tb[1:])
            if not torch.equal(tb[1:-1], want) or int(tb[0]) != GUARD or int(tb[-1]) != GUARD:
                bad.append((kind, lo, ko, int((tb[1:-1] != want).sum())))
        # two halves accumulated = one call; accumulating no rows leaves it; no rows zero it
        h = 7777
        whole = _dev(torch, key_table(lab[:n], key[:n], m, nk).reshape(-1), cuda_dev)
        tb.fill_(GUARD)
        _key_count(lib, torch, lab_d, key_d, h, m, nk, 0, tb[1:])
        _key_count(lib, torch, lab_d[h:], key_d[h:], n - h, m, nk, 1, tb[1:])
        _key_count(lib, torch, lab_d, key_d, 0, m, nk, 5, tb[1:])
        if not torch.equal(tb[1:-1], whole):
            bad.append((kind, "accumulate"))
        if kind == "one-cell":
            assert int(whole.max()) == n == int(whole.sum())
    _key_count(lib, torch, lab_d, key_d, 0, m, nk, 0, tb[1:])
    assert int(tb[1:-1].abs().sum()) == 0 and int(tb[0]) == GUARD and int(tb[-1]) == GUARD
    assert not bad, bad


def test_key_table_past_the_grid_cap(built_lib, cuda_dev):
    """More rows than the capped grid covers at four quads per thread: the grid-strided loop
    runs on.  The constants are the kernel's own (csrc/rae_profile.hpp RAE_CK_*)."""
    import torch
    from rae import _lib
    from rae.evaluation import key_table
    cap_rows = _lib.RAE_CK_GRID * _lib.RAE_CK_BT * _lib.RAE_CK_QPT * 4
    src = open(os.path.join(_lib.CSRC, "rae_profile.hpp")).read()
    for name in ("RAE_CK_GRID", "RAE_CK_BT", "RAE_CK_QPT"):
        assert f"#define {name} {getattr(_lib, name)} " in src, name
    m, nk, n = 100, 481, cap_rows + 2851
    lab, key = count_rows(np.random.RandomState(5), n + 1, m, nk, "zipf")
    lab_d, key_d = _dev(torch, lab, cuda_dev)[1:], _dev(torch, key, cuda_dev)[1:]
    want = _dev(torch, key_table(lab[1:], key[1:], m, nk).reshape(-1), cuda_dev)
    tb = torch.empty(m * nk, dtype=torch.int32, device=cuda_dev)
    _key_count(built_lib, torch, lab_d, key_d, n, m, nk, 0, tb)
    assert torch.equal(tb, want)


# ------------------------------------------------------------------------------ 3. top-k
def _topk_rows(nk, top, g):
    """The rows of one table, every one a case of its own."""
    big, half = 2 ** 31 - 1, 2 ** 30
    ar = np.arange(nk, dtype=np.int64)
    rows = {}
    rows["zero"] = np.zeros(nk, np.int64)
    few = np.zeros(nk, np.int64)
    few[g.choice(nk, size=min(nk, max(top - 1, 1)), replace=False)] = g.randint(1, 9, min(nk, max(top - 1, 1)))
    rows["few"] = few
    rows["equal"] = np.full(nk, 7, np.int64)
    rows["ascending"] = ar + 1
    rows["descending"] = nk - ar
    last = g.randint(0, 50, nk).astype(np.int64)
    last[-1] = 1000
    rows["max-last"] = last
    # ties across the lane (64), wave-round (512) and workgroup-round (8192) boundaries of the
    # kernel: 9s there in a row of 3s, more of them than `top`
    ties = np.full(nk, 3, np.int64)
    for b in (64, 512, 1024, 8192, 16384, nk):
        for o in (-1, 0, 1):
            if 0 <= b + o < nk:
                ties[b + o] = 9
    rows["ties"] = ties
    large = g.randint(0, 3, nk).astype(np.int64) * half          # 0, 2^30 and (capped) 2^31 - 1
    rows["large"] = np.minimum(large, big)
    rows["random"] = np.floor(1.0 / g.random_sample(nk)).astype(np.int64).clip(0, 10 ** 6) * (g.rand(nk) < 0.7)
    return rows


@pytest.mark.parametrize("top", [1, 5, 32])
@pytest.mark.parametrize("nk", [1, 63, 64, 65, 481, 100003])
def test_topk_is_exact(built_lib, cuda_dev, nk, top):
    import torch
    from rae.evaluation import topk_from_table
    g = np.random.RandomState(nk + top)
    rows = _topk_rows(nk, top, g)
    names = list(rows)
    table = np.stack([rows[k] for k in names]).astype(np.int32)
    m = table.shape[0]
    if nk > 2:
        assert table[names.index("large")].max() == 2 ** 31 - 1
        assert (table[names.index("large")] == 2 ** 30).any()
    wk, wc = topk_from_table(table, top)
    assert (wk[names.index("equal")][:min(top, nk)] == np.arange(min(top, nk))).all()
    assert (wk[names.index("zero")] == -1).all()
    for pad in (0, 5):                     # ld == n_keys, and garbage in the padding columns
        ld = nk + pad
        full = np.empty((m, ld), dtype=np.int32)
        full[:, :nk] = table
        full[:, nk:] = [2 ** 31 - 1, -1, 2 ** 30, -(2 ** 31), 12345][:pad]
        tb = _dev(torch, full, cuda_dev)
        out = torch.full((2, m * top + 8), GUARD, dtype=torch.int32, device=cuda_dev)
        rc = built_lib.rae_cluster_topk(_p(tb), m, nk, ld, top, _p(out[0], 4), _p(out[1], 4),
                                        _stream(torch, cuda_dev))
        assert rc == 0, built_lib.rae_last_error()
        host = out.cpu().numpy()
        assert (host[:, :4] == GUARD).all() and (host[:, 4 + m * top:] == GUARD).all()
        gk, gc = host[0, 4:4 + m * top].reshape(m, top), host[1, 4:4 + m * top].reshape(m, top)
        for c, name in enumerate(names):
            assert gk[c].tolist() == wk[c].tolist(), (name, pad)
            assert gc[c].tolist() == wc[c].tolist(), (name, pad)


# ------------------------------------------------------------------------- engine fixtures
def _inducer(data, gold, dev, m=10, r=16, s=4, l=100, epochs=2, seed=2, **kw):
    from rae.inducer import ReconstructInducer
    return ReconstructInducer(data, gold, np.random.RandomState(seed), epochs, 0.1, l, r, m, s,
                              0.0, 0.0, "adagrad", "pf", "sp", False, True, False, 1.0,
                              device=dev, graph_chunk=8, **kw)


def _same_params(a, b):
    import torch
    pa, pb = a.modelFunc.named_params(), b.modelFunc.named_params()
    return all(torch.equal(pa[k], pb[k]) for k in pa)


def _oracle_profiles(eng, split, host_x, ki, row0, nrows, top):
    from rae.evaluation import key_table, row_keys, topk_from_table
    lab = eng.label(split, row0, nrows, probs=False)[0].cpu().numpy() if nrows else np.zeros(0, np.int64)
    keys = ki.rows if ki.rows is not None else row_keys(host_x, ki.key_of_feature)
    table = key_table(lab, keys[row0:row0 + nrows], eng.m, ki.n_keys)
    return topk_from_table(table, top), table


# --------------------------------------------------------------------------- 4. end to end
def test_engine_cluster_profiles_on_the_sample(built_lib, cuda_dev):
    """The sample, m = 10, after two epochs: cluster_profiles = the numpy oracle on the
    downloaded labels, for the lexicon's triggers and for the gold labels."""
    from rae.evaluation import GoldIndex, KeyIndex
    data, gold = sample_data()
    ind = _inducer(data, gold, cuda_dev, r=10, s=5)
    ind.learn(verbose=False)
    eng, sp_ = ind.engine, ind.engine.split
    X = data.split["train"].xFeats
    ki = KeyIndex.from_lexicon(data.featureLex)
    for k, r0, n, top in ((ki, 0, 1000, 5), (ki, 37, 901, 32), (ki, 999, 1, 1), (ki, 10, 0, 5),
                          (KeyIndex.from_gold(gold["train"], 1000), 0, 1000, 5)):
        res = eng.cluster_profiles(sp_, k, r0, n, top)
        (wk, wc), table = _oracle_profiles(eng, sp_, X, k, r0, n, top)
        assert res.keys.dtype == res.counts.dtype == np.int32
        assert np.array_equal(res.keys, wk) and np.array_equal(res.counts, wc)
        assert np.array_equal(eng._pf_table[:eng.m * k.n_keys].cpu().numpy().reshape(eng.m, -1),
                              table)
        assert table.sum() == n
    assert len(set(eng.label(sp_, 0, 1000, probs=False)[0].cpu().tolist())) > 1
    # the row keys are computed once per (split, key index)
    assert eng._keys_dev(sp_, ki) is eng._keys_dev(sp_, ki)
    # the combined path: one labelling pass, the same metrics and profiles
    gi = GoldIndex(gold["train"], sp_.N)
    both = eng.cluster_metrics_and_profiles(sp_, gi, ki, 0, 1000, 5)
    alone = eng.cluster_metrics(sp_, gi, 0, 1000)
    assert both[0][:4] == alone[:4] and np.array_equal(both[0].sizes, alone.sizes)
    (wk, wc), _ = _oracle_profiles(eng, sp_, X, ki, 0, 1000, 5)
    assert np.array_equal(both[1].keys, wk) and np.array_equal(both[1].counts, wc)
    with pytest.raises(RuntimeError):          # the mark is consumed: no stale labels
        eng.queue_cluster_profiles(sp_, ki, 0, 1000, 5, reuse_labels=True)
    with pytest.raises(IndexError):
        eng.cluster_profiles(sp_, ki, 10, 1000)
    with pytest.raises(ValueError):
        eng.cluster_profiles(sp_, ki, top=33)
    eng.close()


def test_label_count_b3_keycount_topk_graph(built_lib, cuda_dev):
    """label -> count -> b3 -> key count -> top-k captured into one HIP graph: the replay gives
    the eager results bit for bit, and after W changed those of the new W."""
    import torch
    from rae.data import synthetic_dataset
    from rae.evaluation import GoldIndex, KeyIndex
    data, gold = synthetic_dataset(20000, 4000, 10, seed=7, gold_fraction=0.05)
    ind = _inducer(data, gold, cuda_dev)
    ind.compile_function()
    eng = ind.engine
    gi = GoldIndex(gold["train"], eng.split.N)
    ki = KeyIndex.from_mask(np.random.RandomState(9).rand(4000) < 0.15)
    X = data.split["train"].xFeats
    n, top = 4999, 5

    def queue():
        eng.queue_cluster_metrics(eng.split, gi, 3, n)
        eng.queue_cluster_profiles(eng.split, ki, 3, n, top, reuse_labels=True)

    def snapshot():
        torch.cuda.synchronize()
        half = eng._pf_out.numel() // 2                     # the words the top-k call writes
        return (eng._cl_out.clone(), eng._pf_table[:eng.m * ki.n_keys].clone(),
                eng._pf_out[:eng.m * top].clone(), eng._pf_out[half:half + eng.m * top].clone())

    def dirty():
        for t in (eng._cl_out, eng._cl_table, eng._pf_table, eng._pf_out, eng._cl_labels):
            t.fill_(5)

    queue()                                                 # eager (and the allocations)
    eager = snapshot()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(cuda_dev)
    s.wait_stream(torch.cuda.current_stream(cuda_dev))
    with torch.cuda.graph(g, stream=s):
        queue()
    torch.cuda.current_stream(cuda_dev).wait_stream(s)
    dirty()
    g.replay()
    got = snapshot()
    assert all(torch.equal(a, b) for a, b in zip(got, eager))
    assert 0 < int(eager[1].sum()) <= n
    W = ind.modelFunc.params[0]
    W.copy_(torch.randn(W.shape, generator=torch.Generator(device="cpu").manual_seed(3)).to(cuda_dev))
    dirty()
    g.replay()
    got2 = snapshot()
    assert not torch.equal(got2[1], eager[1])
    (wk, wc), table = _oracle_profiles(eng, eng.split, X, ki, 3, n, top)
    assert np.array_equal(got2[1].cpu().numpy().reshape(eng.m, -1), table)
    res = eng._profile_result(top)
    assert np.array_equal(res.keys, wk) and np.array_equal(res.counts, wc)
    eng.close()


def _strip(out):
    return [ln for ln in out.splitlines() if not ln.startswith("Epoch duration")]


def test_learn_prints_the_same_profiles_from_host_and_device(built_lib, cuda_dev, capsys):
    import torch
    data, gold = sample_data()
    runs = {}
    for tag, kw in (("off", {}),
                    ("host", dict(print_clusters="host")),
                    ("device", dict(print_clusters="device")),
                    ("device-both", dict(print_clusters="device", cluster_eval="device")),
                    ("gold-host", dict(print_clusters="host", print_by="gold", print_top=3)),
                    ("gold-device", dict(print_clusters="device", print_by="gold", print_top=3))):
        ind = _inducer(data, gold, cuda_dev, r=10, s=5, **kw)
        ind.learn(verbose=True)
        torch.cuda.synchronize()
        runs[tag] = (ind, _strip(capsys.readouterr().out))
    off_ind, off = runs["off"]
    # print_clusters="off": exactly the lines learn() printed before the option existed
    want = []
    for e, err in enumerate(off_ind.train_errors):
        want += ["", f"EPOCH {e + 1}", "Training error: {:.4f}".format(err)]
        want.append(off[len(want)])
        assert re.fullmatch(r"train f1: \d\.\d{4} pre: \d\.\d{4} rec: \d\.\d{4}", want[-1])
    assert off == want and len(off) == 8
    host = runs["host"][1]
    assert host == runs["device"][1] == runs["device-both"][1]
    assert runs["gold-host"][1] == runs["gold-device"][1] != host
    # the profile lines follow each f1 line: one per cluster id, the rest is the `off` output
    m = 10
    assert len(host) == len(off) + 2 * m
    blocks = [i + 1 for i, ln in enumerate(host) if ln.startswith("train f1: ")]
    assert len(blocks) == 2
    for b in blocks:
        block = host[b:b + m]
        assert [ln.split(" ", 1)[0] for ln in block] == [str(c) for c in range(m)]
        assert any(re.search(r"\('.+', \d+\)", ln) for ln in block)
    assert [ln for ln in host if not re.match(r"\d+ ", ln)] == off
    for tag in runs:
        assert _same_params(runs[tag][0], off_ind), tag
        runs[tag][0].engine.close()
