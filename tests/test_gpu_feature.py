"""Relation feature profiles on the device (rae_feature_support / rae_feature_topk, include/rae.h;
TrainEngine.feature_support / relation_features; ReconstructInducer(print_features=...)) against
the numpy oracles of rae/evaluation.py, which tests/test_feature_host.py pins to explicit loops.
Exact equality throughout: the supports are integers, the order is total, and the centred scores
are compared bit for bit.

The partitioned (two-rank) form is left out: the two-rank fixture of tests/test_dist.py drives a
worker script with fixed modes, and relation_features takes the same replica sync in front of it
that label takes there."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from _profile_sample import sample_data

pytestmark = pytest.mark.gpu

GUARD = -7
GUARD_F = -77.0


def _p(t, off=0):
    """The tensor's device address (from its storage: an empty view's data_ptr() is 0)."""
    if t is None:
        return None
    return C.c_void_p(t.untyped_storage().data_ptr() + (t.storage_offset() + off) * t.element_size())


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(torch, a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


# --------------------------------------------------------------------------- 1. the support
def _cycling_csr(seed, n, d, hot=None):
    """Row lengths cycling {0, 1, 17, 64, 65, 130}, ~15 % of the stored values 0; `hot`: that
    feature is stored (non-zero) in every row besides."""
    g = np.random.RandomState(seed)
    lengths = [0, 1, 17, 64, 65, 130]
    indptr, idx, val = [0], [], []
    for i in range(n):
        cols = np.sort(g.choice(d, size=lengths[i % 6], replace=False))
        v = np.where(g.rand(cols.shape[0]) < 0.15, 0.0, 1.0 + (g.rand(cols.shape[0]) < 0.3))
        if hot is not None:
            keep = cols != hot
            cols, v = np.append(cols[keep], hot), np.append(v[keep], 1.0)
        idx.extend(cols.tolist())
        val.extend(v.tolist())
        indptr.append(len(idx))
    return sp.csr_matrix((np.array(val, np.float32), np.array(idx, np.int32),
                          np.array(indptr, np.int32)), shape=(n, d))


class _Csr:
    """A CSR in HBM; voff: the values start voff floats into their buffer (voff % 4 != 0: they are
    not aligned where the indices are -- the kernel reads them as dwords)."""

    def __init__(self, torch, dev, X, voff=0):
        self.X, self.torch, self.dev = X, torch, dev
        self.ip = _dev(torch, X.indptr.astype(np.int32), dev)
        self.ix = _dev(torch, X.indices.astype(np.int32), dev)
        buf = np.zeros(X.nnz + voff, np.float32)
        buf[voff:] = X.data
        self.vv = _dev(torch, buf, dev)[voff:]

    def support(self, lib, n_features, row0, nrows, values=True, acc=0, out=None):
        """One call into a guarded buffer (given: accumulate into it); the words written."""
        torch = self.torch
        if out is None:
            out = torch.full((n_features + 8,), GUARD, dtype=torch.int32, device=self.dev)
        rc = lib.rae_feature_support(_p(self.ip), _p(self.ix), _p(self.vv) if values else None,
                                     n_features, row0, nrows, acc, _p(out, 4),
                                     _stream(torch, self.dev))
        assert rc == 0, lib.rae_last_error()
        host = out.cpu().numpy()
        assert (host[:4] == GUARD).all() and (host[4 + n_features:] == GUARD).all()
        return host[4:4 + n_features], out


def _want_support(X, n_features, row0, nrows, values=True):
    from rae.evaluation import feature_support
    return feature_support(X[row0:row0 + nrows], use_values=values, n_features=n_features)


@pytest.mark.parametrize("voff", [0, 1], ids=["values-aligned", "values-by-dwords"])
def test_support_is_exact(built_lib, cuda_dev, voff):
    import torch
    n, d = 1500, 3000
    X = _cycling_csr(4, n, d)
    assert set(np.diff(X.indptr).tolist()) == {0, 1, 17, 64, 65, 130}
    assert 0.1 < (X.data == 0).mean() < 0.2
    csr = _Csr(torch, cuda_dev, X, voff)
    for values in (True, False):
        want = _want_support(X, d, 0, n, values)
        assert np.array_equal(csr.support(built_lib, d, 0, n, values)[0], want)
        # row sub-ranges (the nnz stream then starts at every alignment), a single row, no rows
        for r0, k in ((37, 101), (1, 7), (2, 6), (3, 601), (n - 1, 1), (n - 6, 6), (6, 1)):
            got = csr.support(built_lib, d, r0, k, values)[0]
            assert np.array_equal(got, _want_support(X, d, r0, k, values)), (r0, k, values)
        assert (csr.support(built_lib, d, 37, 0, values)[0] == 0).all()      # still zeroed
        # two halves accumulated = one call; accumulating no rows leaves it
        _, out = csr.support(built_lib, d, 0, 777, values)
        _, out = csr.support(built_lib, d, 777, n - 777, values, acc=1, out=out)
        got, _ = csr.support(built_lib, d, 5, 0, values, acc=5, out=out)
        assert np.array_equal(got, want)
        # columns at and past n_features are skipped (and support is not written there)
        for nf in (2000, 1, 0):
            got = csr.support(built_lib, nf, 0, n, values)[0]
            assert np.array_equal(got, _want_support(X, nf, 0, n, values)), nf
    assert (_want_support(X, d, 0, n, True) != _want_support(X, d, 0, n, False)).any()
    assert X.indices.max() >= 2000


def test_support_hot_cell_and_more_features_than_slots(built_lib, cuda_dev):
    """One feature in every row (every workgroup adds to one cell; with nothing else in the rows,
    every lane of a wave instruction does), and more distinct features per workgroup than the LDS
    aggregation has slots
    (csrc/rae_profile.hpp RAE_CK_SLOT_BITS 12: 4096; the grid is sized at RAE_FS_ROWS 32 rows per
    workgroup, so 2000 rows of 150 entries give a workgroup ~4700 entries of 20000 features)."""
    import torch
    from rae import _lib
    src = open(os.path.join(_lib.CSRC, "rae_profile.hpp")).read()
    assert "#define RAE_CK_SLOT_BITS 12 " in src
    assert "#define RAE_FS_ROWS 32 " in open(os.path.join(_lib.CSRC, "rae_feature.hpp")).read()
    hot = _cycling_csr(5, 1200, 500, hot=123)
    want = _want_support(hot, 500, 0, 1200)
    assert want[123] == 1200
    assert np.array_equal(_Csr(torch, cuda_dev, hot).support(built_lib, 500, 0, 1200)[0], want)
    only = sp.csr_matrix((np.ones(5000, np.float32), np.full(5000, 7, np.int32),
                          np.arange(5001, dtype=np.int32)), shape=(5000, 9))
    got = _Csr(torch, cuda_dev, only).support(built_lib, 9, 0, 5000)[0]
    assert got.tolist() == [0] * 7 + [5000, 0]
    g = np.random.RandomState(6)
    n, d, L = 2000, 20000, 150
    idx = np.stack([np.sort(g.choice(d, size=L, replace=False)) for _ in range(n)]).reshape(-1)
    wide = sp.csr_matrix((np.ones(n * L, np.float32), idx.astype(np.int32),
                          np.arange(0, n * L + 1, L, dtype=np.int32)), shape=(n, d))
    want = _want_support(wide, d, 0, n)
    # the quads workgroup 0 meets in its grid-strided loop (RAE_FS_BT 256 threads; the stream
    # starts 16-byte aligned): more distinct features than slots
    q = np.arange(n * L // 4)
    mine = idx.reshape(-1, 4)[(q % (-(-n // 32) * 256)) < 256]
    assert np.unique(mine).shape[0] > 4096
    assert np.array_equal(_Csr(torch, cuda_dev, wide).support(built_lib, d, 0, n)[0], want)


# ------------------------------------------------------------------------------ 2. top-k
class _Ftopk:
    """rae_feature_topk through the C ABI with guard words around both outputs and a workspace
    of exactly the bytes the sizing call asks for."""

    def __init__(self, lib, torch, dev):
        self.lib, self.torch, self.dev = lib, torch, dev

    def args(self, W, d, m, ldw, support, min_support, centre, top):
        from rae import _lib
        a = _lib.RaeFtopkArgs()
        a.W = _p(W) if d else None
        a.n_features, a.relations, a.ldw = d, m, ldw
        a.support = _p(support)
        a.min_support, a.centre, a.top = min_support, int(centre), top
        need = self.lib.rae_feature_topk_workspace_bytes(C.byref(a))
        assert need >= 0, self.lib.rae_last_error()
        ws = self.torch.full((need + 512,), 0x5A, dtype=self.torch.uint8, device=self.dev)
        a.workspace, a.workspace_bytes = _p(ws, 256 - ws.data_ptr() % 256), need
        return a, ws, need

    def __call__(self, W, d, m, ldw=None, support=None, min_support=0, centre=True, top=5):
        torch = self.torch
        a, ws, need = self.args(W, d, m, m if ldw is None else ldw, support, min_support, centre, top)
        fo = torch.full((m * top + 8,), GUARD, dtype=torch.int32, device=self.dev)
        so = torch.full((m * top + 8,), GUARD_F, dtype=torch.float32, device=self.dev)
        a.feats_out, a.scores_out = _p(fo, 4), _p(so, 4)
        rc = self.lib.rae_feature_topk(C.byref(a), _stream(torch, self.dev))
        assert rc == 0, self.lib.rae_last_error()
        f, s, w = fo.cpu().numpy(), so.cpu().numpy(), ws.cpu().numpy()
        assert (f[:4] == GUARD).all() and (f[4 + m * top:] == GUARD).all()
        assert (s[:4] == GUARD_F).all() and (s[4 + m * top:] == GUARD_F).all()
        o = 256 - ws.data_ptr() % 256                         # nothing outside the workspace
        assert (w[:o] == 0x5A).all() and (w[o + need:] == 0x5A).all()
        return f[4:4 + m * top].reshape(m, top), s[4:4 + m * top].reshape(m, top)


def _cut(ref, top):
    """The oracle at top = 32 cut to `top`: the order is total, so a shorter list is a prefix."""
    return ref[0][:, :top], ref[1][:, :top]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and \
        np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


M_SMALL = [1, 3, 63, 64, 65, 100, 128, 130, 512]
D_SMALL = [1, 5, 63, 64, 65, 1000, 4097]


@pytest.mark.parametrize("m", M_SMALL)
def test_topk_small_integers(built_lib, cuda_dev, m):
    """W in {-2..2}: massive ties, the feature-ascending rule decides; at m a power of two the
    centred means are exact.  Every d, top in {1, 5, 32} (top > d and top > the eligible count
    among them), centred and raw."""
    import torch
    from rae.evaluation import feature_topk
    run = _Ftopk(built_lib, torch, cuda_dev)
    bad = []
    for d in D_SMALL:
        g = np.random.RandomState(1000 * m + d)
        W = g.randint(-2, 3, (d, m)).astype(np.float32)
        sup = g.randint(0, 4, d).astype(np.int32)
        Wd, sd = _dev(torch, W, cuda_dev), _dev(torch, sup, cuda_dev)
        for centre in (True, False):
            ref = feature_topk(W, None, 0, centre, 32)
            ref3 = feature_topk(W, sup, 3, centre, 32)        # about a quarter eligible
            for top in (1, 5, 32):
                if not _same(run(Wd, d, m, centre=centre, top=top), _cut(ref, top)):
                    bad.append((d, centre, top, "all"))
                if not _same(run(Wd, d, m, support=sd, min_support=3, centre=centre, top=top),
                             _cut(ref3, top)):
                    bad.append((d, centre, top, "support"))
    assert not bad, bad


def test_topk_at_the_kernels_seams(built_lib, cuda_dev):
    """d one below, at and one above the selection kernel's own steps (csrc/rae_feature.hpp): the
    rows of a workgroup step RAE_FT_WAVES * RAE_FT_U = 64, the shortest strip RAE_FT_STRIP_ROWS =
    512 (1 -> 2 strips; 1024: 2 -> 3), and RAE_FT_MAXSTRIPS * RAE_FT_STRIP_ROWS = 65536, where the
    strip count stops at 128 and the strips grow instead."""
    import torch
    from rae import _lib
    from rae.evaluation import feature_topk
    src = open(os.path.join(_lib.CSRC, "rae_feature.hpp")).read()
    for name in ("RAE_FT_WAVES", "RAE_FT_U", "RAE_FT_STRIP_ROWS", "RAE_FT_MAXSTRIPS"):
        assert re.search(rf"#define {name} {getattr(_lib, name)}\s", src), name
    step = _lib.RAE_FT_WAVES * _lib.RAE_FT_U
    strip, cap = _lib.RAE_FT_STRIP_ROWS, _lib.RAE_FT_MAXSTRIPS * _lib.RAE_FT_STRIP_ROWS
    assert (step, strip, cap) == (64, 512, 65536)
    assert [_lib.ftopk_strips(x) for x in (strip, strip + 1, 2 * strip, 2 * strip + 1, cap, cap + 1)] \
        == [1, 2, 2, 3, 128, 128]
    assert _lib.ftopk_strip_rows(cap) == strip and _lib.ftopk_strip_rows(cap + 1) == strip + step
    run = _Ftopk(built_lib, torch, cuda_dev)
    bad = []
    for d in (step - 1, step, step + 1, strip - 1, strip, strip + 1, 2 * strip - 1, 2 * strip,
              2 * strip + 1, cap - 1, cap, cap + 1):
        g = np.random.RandomState(d)
        for m in ((5, 65) if d < cap - 1 else (5,)):
            W = g.randint(-2, 3, (d, m)).astype(np.float32)
            W[d - 1, :] = 3.0                                  # the last row wins every column
            Wd = _dev(torch, W, cuda_dev)
            for centre in (True, False):
                ref = feature_topk(W, None, 0, centre, 32)
                for top in (1, 32):
                    if not _same(run(Wd, d, m, centre=centre, top=top), _cut(ref, top)):
                        bad.append((d, m, centre, top))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["normal", "scaled"])
def test_topk_floats_bit_for_bit(built_lib, cuda_dev, kind):
    """Float W (normal; normal scaled by 10^+-3 per row): the centred scores equal the oracle's bit
    for bit, which pins the summation order and the single rounding.  Rows with a NaN, +inf, -inf
    and -0.0 among them."""
    import torch
    from rae.evaluation import feature_scores, feature_topk
    run = _Ftopk(built_lib, torch, cuda_dev)
    bad = []
    for d, m in ((1500, 100), (700, 130), (4097, 3), (300, 512), (2000, 64)):
        g = np.random.RandomState(d + m)
        W = g.standard_normal((d, m)).astype(np.float32)
        if kind == "scaled":
            W *= np.power(10.0, g.randint(-3, 4, (d, 1))).astype(np.float32)
        rows = g.choice(d, size=8, replace=False)
        W[rows[0], g.randint(m)] = np.nan
        W[rows[1], g.randint(m)] = np.inf
        W[rows[2], g.randint(m)] = -np.inf
        W[rows[3], :] = -0.0
        W[rows[4], :] = 0.0
        W[rows[5], 0] = -0.0
        W[rows[6], 0], W[rows[6], m - 1] = np.inf, -np.inf
        W[rows[7], :] = np.inf
        Wd = _dev(torch, W, cuda_dev)
        for centre in (True, False):
            ref = feature_topk(W, None, 0, centre, 32)
            for top in (1, 10, 32):
                got = run(Wd, d, m, centre=centre, top=top)
                if not _same(got, _cut(ref, top)):
                    bad.append((d, m, centre, top))
        # the oracle's centred scores are not the plain float32 expression's: the test can tell
        s = feature_scores(W, True)
        plain = W - W.mean(axis=1, dtype=np.float32, keepdims=True)
        fin = np.isfinite(s) & np.isfinite(plain)
        assert (s[fin] != plain[fin]).any()
    assert not bad, bad


def test_topk_support_filter(built_lib, cuda_dev):
    import torch
    from rae.evaluation import feature_topk
    run = _Ftopk(built_lib, torch, cuda_dev)
    g = np.random.RandomState(8)
    d, m = 3000, 10
    W = g.standard_normal((d, m)).astype(np.float32)
    sup = np.minimum(g.zipf(1.5, d), 1000).astype(np.int32)
    sup[::7] = 0
    Wd, sd = _dev(torch, W, cuda_dev), _dev(torch, sup, cuda_dev)
    assert 0.1 < (sup >= 5).mean() < 0.9
    for centre in (True, False):
        for ms in (5, 1, 0, -3):
            want = feature_topk(W, sup, ms, centre, 32)
            assert _same(run(Wd, d, m, support=sd, min_support=ms, centre=centre, top=32), want), ms
            assert (sup[want[0]] >= ms).all()
        # support NULL: min_support is ignored
        want = feature_topk(W, None, 0, centre, 32)
        assert _same(run(Wd, d, m, support=None, min_support=10 ** 6, centre=centre, top=32), want)
        # every feature ineligible: all padding; fewer eligible than top: padded
        f, s = run(Wd, d, m, support=sd, min_support=1001, centre=centre, top=5)
        assert (f == -1).all() and (s == -np.inf).all()
        few = np.zeros(d, np.int32)
        few[[5, 2999, 1024]] = 9
        want = feature_topk(W, few, 9, centre, 5)
        assert (want[0][:, 3:] == -1).all() and (want[0][:, :3] >= 0).all()
        assert _same(run(Wd, d, m, support=_dev(torch, few, cuda_dev), min_support=9, centre=centre,
                         top=5), want)
    # no feature at all: all padding, W is not read
    f, s = run(None, 0, 7, centre=True, top=4)
    assert f.shape == (7, 4) and (f == -1).all() and (s == -np.inf).all()
    # scores_out may be NULL
    a, ws, _ = run.args(Wd, d, m, m, None, 0, 1, 5)
    fo = torch.full((m * 5,), GUARD, dtype=torch.int32, device=cuda_dev)
    a.feats_out, a.scores_out = _p(fo), None
    assert built_lib.rae_feature_topk(C.byref(a), _stream(torch, cuda_dev)) == 0
    assert np.array_equal(fo.cpu().numpy().reshape(m, 5), feature_topk(W, None, 0, True, 5)[0])


def test_topk_strided_and_unaligned_w(built_lib, cuda_dev):
    """ldw > m: columns [m, ldw) hold NaN and never show, nor enter a row sum; a W base that is
    only float-aligned."""
    import torch
    from rae.evaluation import feature_topk
    run = _Ftopk(built_lib, torch, cuda_dev)
    g = np.random.RandomState(12)
    for d, m, ldw, off in ((777, 100, 128, 0), (600, 3, 5, 1), (1025, 64, 67, 3), (513, 130, 130, 1)):
        W = g.standard_normal((d, m)).astype(np.float32)
        full = np.full(d * ldw + 4, np.nan, np.float32)
        full[off:off + d * ldw].reshape(d, ldw)[:, :m] = W
        Wd = _dev(torch, full, cuda_dev)[off:]
        for centre in (True, False):
            want = feature_topk(W, None, 0, centre, 7)
            assert _same(run(Wd, d, m, ldw=ldw, centre=centre, top=7), want), (d, m, ldw, centre)


def test_topk_rows_past_2_31_elements(built_lib, cuda_dev):
    """m = 4, ldw = 512, d just above 2^22: the last rows lie past 2^31 elements (8 GiB of address
    range; only the (d, 4) view is written).  Planted winners in the last rows; every other row
    is -1, so the rest of a list is the lowest feature ids."""
    import torch
    from rae.evaluation import feature_topk
    m, ldw, d = 4, 512, (1 << 22) + 77
    assert (d - 1) * ldw > 2 ** 31
    try:
        buf = torch.empty(d * ldw, dtype=torch.float32, device=cuda_dev)
    except RuntimeError as e:                                   # out of memory on a shared card
        pytest.skip(f"cannot allocate {d * ldw * 4 >> 30} GiB: {e}")
    view = buf.view(d, ldw)[:, :m]
    view.fill_(-1.0)
    g = np.random.RandomState(13)
    planted = np.concatenate([d - 1 - np.arange(6), [(1 << 22) + 1, (1 << 22) - 1, 12345]])
    vals = g.standard_normal((planted.shape[0], m)).astype(np.float32) + 3.0
    view[torch.as_tensor(planted, device=cuda_dev)] = _dev(torch, vals, cuda_dev)
    # the oracle on the rows that can appear: the planted ones and the 32 lowest ids
    rows = np.unique(np.concatenate([planted, np.arange(32)]))
    sub = np.full((rows.shape[0], m), -1.0, np.float32)
    sub[np.searchsorted(rows, planted)] = vals
    run = _Ftopk(built_lib, torch, cuda_dev)
    for centre in (True, False):
        wf, wsc = feature_topk(sub, None, 0, centre, 32)
        want = (rows[wf].astype(np.int32), wsc)
        got = run(buf, d, m, ldw=ldw, centre=centre, top=32)
        assert _same(got, want), centre
        if not centre:                                          # every planted row beats -1
            assert all(set(planted.tolist()) <= set(row.tolist()) for row in got[0])
    del buf, view


def test_topk_rows_are_independent(built_lib, cuda_dev):
    """A relation's row: the same when the other columns change (raw; centred when they change
    without changing the row sums), when top grows (a prefix), when the call repeats, and inside a
    captured graph replayed twice."""
    import torch
    from rae.evaluation import feature_topk
    run = _Ftopk(built_lib, torch, cuda_dev)
    g = np.random.RandomState(14)
    d, m, k = 2500, 70, 41
    W = g.standard_normal((d, m)).astype(np.float32)
    other = W.copy()
    keep = np.arange(m) == k
    other[:, ~keep] = g.standard_normal((d, m - 1)).astype(np.float32) * 5
    a = run(_dev(torch, W, cuda_dev), d, m, centre=False, top=9)
    b = run(_dev(torch, other, cuda_dev), d, m, centre=False, top=9)
    assert _same((a[0][k], a[1][k]), (b[0][k], b[1][k])) and not np.array_equal(a[0], b[0])
    Wi = g.randint(-2, 3, (d, m)).astype(np.float32)            # integers: the sums are exact
    perm = np.arange(m)
    perm[~keep] = np.roll(perm[~keep], 5)
    a = run(_dev(torch, Wi, cuda_dev), d, m, centre=True, top=9)
    b = run(_dev(torch, Wi[:, perm], cuda_dev), d, m, centre=True, top=9)
    assert _same((a[0][k], a[1][k]), (b[0][k], b[1][k]))
    Wd = _dev(torch, W, cuda_dev)
    for centre in (True, False):
        long = run(Wd, d, m, centre=centre, top=32)
        assert _same(long, feature_topk(W, None, 0, centre, 32))
        for top in (1, 9):
            assert _same(run(Wd, d, m, centre=centre, top=top), _cut(long, top))
        assert _same(run(Wd, d, m, centre=centre, top=32), long)                 # the call repeats
        # captured: the replay gives the eager result, and after W changed that of the new W
        Wg = Wd.clone()
        args, ws, _ = run.args(Wg, d, m, m, None, 0, centre, 32)
        fo = torch.full((m * 32,), GUARD, dtype=torch.int32, device=cuda_dev)
        so = torch.full((m * 32,), GUARD_F, dtype=torch.float32, device=cuda_dev)
        args.feats_out, args.scores_out = _p(fo), _p(so)
        s = torch.cuda.Stream(cuda_dev)
        s.wait_stream(torch.cuda.current_stream(cuda_dev))
        with torch.cuda.stream(s):                              # the large-LDS opt-in, eagerly
            assert built_lib.rae_feature_topk(C.byref(args), _stream(torch, cuda_dev)) == 0
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            rc = built_lib.rae_feature_topk(C.byref(args), _stream(torch, cuda_dev))
        assert rc == 0, built_lib.rae_last_error()
        torch.cuda.current_stream(cuda_dev).wait_stream(s)
        for rep in range(2):
            fo.fill_(GUARD)
            so.fill_(GUARD_F)
            ws.fill_(0x33)
            graph.replay()
            torch.cuda.synchronize()
            assert _same((fo.cpu().numpy().reshape(m, 32), so.cpu().numpy().reshape(m, 32)), long)
        Wg.copy_(_dev(torch, other, cuda_dev))
        graph.replay()
        torch.cuda.synchronize()
        assert _same((fo.cpu().numpy().reshape(m, 32), so.cpu().numpy().reshape(m, 32)),
                     feature_topk(other, None, 0, centre, 32))
        del graph


# --------------------------------------------------------------------------- 3. end to end
def _inducer(data, gold, dev, m=10, r=10, s=5, l=100, epochs=2, seed=2, **kw):
    from rae.inducer import ReconstructInducer
    return ReconstructInducer(data, gold, np.random.RandomState(seed), epochs, 0.1, l, r, m, s,
                              0.0, 0.0, "adagrad", "pf", "sp", False, True, False, 1.0,
                              device=dev, graph_chunk=8, **kw)


def test_engine_and_inducer_on_the_sample(built_lib, cuda_dev, capsys):
    """After two epochs on the sample: relation_features = the oracle on the downloaded W and the
    split's CSR, and the lines learn() prints = format_relation_features of the oracle's result
    with the lexicon's strings."""
    import torch
    from rae.evaluation import feature_support, feature_topk, format_relation_features
    data, gold = sample_data()
    X = data.split["train"].xFeats
    ind = _inducer(data, gold, cuda_dev, print_features=5, print_features_min_count=3)
    ind.learn(verbose=True)
    torch.cuda.synchronize()
    out = capsys.readouterr().out.splitlines()
    eng = ind.engine
    W = ind.modelFunc.params[0].detach().cpu().numpy()
    sup = feature_support(X)
    got_sup = eng.feature_support(eng.split)
    assert got_sup.dtype == torch.int32 and np.array_equal(got_sup.cpu().numpy()[:X.shape[1]], sup)
    assert eng.feature_support(eng.split) is got_sup                # once per split
    for top, centre, ms, split in ((5, True, 3, eng.split), (32, False, 0, eng.split),
                                   (10, True, 0, None), (1, False, 10 ** 6, eng.split),
                                   (7, False, 10 ** 6, None)):
        f, s = eng.relation_features(top=top, centre=centre, min_support=ms, split=split)
        assert f.shape == s.shape == (eng.m, top) and f.dtype == torch.int32
        want = feature_topk(W, None if split is None else sup, ms, centre, top)
        assert _same((f.cpu().numpy(), s.cpu().numpy()), want), (top, centre, ms)
    with pytest.raises(ValueError):
        eng.relation_features(top=33)
    # the printed lines: the last epoch's are those of the final W
    want = format_relation_features(*feature_topk(W, sup, 3, True, 5), sup,
                                    data.featureLex.get_str_pruned)
    lines = [ln for ln in out if ln.startswith("relation ")]
    assert len(lines) == 2 * eng.m and lines[eng.m:] == want
    assert lines[eng.m:] == ind.relation_feature_lines()
    assert any("(" in ln for ln in want)
    # the option changes nothing else: the same parameters as a run without it
    ref = _inducer(data, gold, cuda_dev)
    ref.learn(verbose=False)
    pa, pb = ind.modelFunc.named_params(), ref.modelFunc.named_params()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    ref.engine.close()
    eng.close()


def test_cli_prints_m_lines_per_evaluation(built_lib, cuda_dev, tmp_path, capsys):
    """python -m rae on the sample with --print-features 5: m lines per evaluation, names from the
    lexicon, the last block the final W's; --print-features-raw ranks by W itself."""
    import gzip
    import shutil
    import torch
    from _profile_sample import SAMPLE
    from rae import cli
    from rae import preprocess as P
    from rae.evaluation import feature_support, feature_topk, format_relation_features
    plain, out = str(tmp_path / "data-sample.txt"), str(tmp_path / "ds.json.gz")
    with gzip.open(SAMPLE, "rb") as src, open(plain, "wb") as dst:
        shutil.copyfileobj(src, dst)
    P.preprocess(plain, out)
    capsys.readouterr()
    m, epochs = 6, 2
    base = [out, "--model-name", "m", "--decoder", "sp", "--relations", str(m), "--epochs",
            str(epochs), "--embed-size", "10", "--neg-samples", "5", "--batch-size", "50"]
    for extra, centre, ms, top in ((["--print-features", "5"], True, 5, 5),
                                   (["--print-features", "--print-features-raw",
                                     "--print-features-min-count", "2"], False, 2, 10)):
        ind = cli.main(base + extra)
        torch.cuda.synchronize()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("relation ")]
        assert len(lines) == epochs * m
        W = ind.modelFunc.params[0].detach().cpu().numpy()
        sup = feature_support(ind.data.split["train"].xFeats)
        wf, ws = feature_topk(W, sup, ms, centre, top)
        want = format_relation_features(wf, ws, sup, ind.data.featureLex.get_str_pruned)
        assert lines[-m:] == want and (wf >= 0).all()                 # `top` items on every line
        ind.engine.close()
