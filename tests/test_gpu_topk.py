"""Top-k entity retrieval (rae_topk_queries, rae_eval_topk, TrainEngine.topk_entities /
predict_arguments / relation_preferences, --print-preferences) on an MI355X.

References: rae.evaluation.topk_from_scores (numpy lexsort, pinned on hand cases by
tests/test_topk_host.py) on the float64 product for small-integer inputs, where every fp32
operation is exact and the output must be equal; rae_rank_queries for the score bits; the
float64 restatement of tests/_rank_ref.py for rae_eval_topk, compared through a band around the
cut with test_gpu_eval's tolerances (tests/_topk_ref.py), the leniency capped on the reference
alone.
"""
import ctypes as C
import gzip
import os
import shutil

import numpy as np
import pytest

from _entry_ref import DeviceEval, EvalProblem
from _rank_ref import queries64, rank_queries, scores64
from _topk_ref import (DeviceTopk, assert_band_cap, bits, check_topk_against_float64,
                       topk_queries)
from test_gpu_eval import _inducer, _params

pytestmark = pytest.mark.gpu

# the kernel's seams (csrc/rae_topk.hpp, csrc/rae_rank.hpp): a 32 x 32 MFMA tile, 64 entities per
# entity wave, 128 entities per tile, one strip up to 128 tiles and two tiles a strip beyond, the
# `top` cut, and the round of 1024 queries
TE, MAXSTRIPS, QROUND, ROWCHUNK = 128, 128, 1024, 2048
EXACT_N = [1, 15, 17, 31, 32, 33, 64, 65, 127, 128, 129, 257, 385]
STRIP_SEAM_N = TE * MAXSTRIPS + 1
EXACT_NQ = [0, 1, 17, 130]
TOPS = [1, 5, 32]


def test_constants_are_the_kernels():
    from rae import _lib
    assert (_lib.RAE_RK_TE, _lib.RAE_RK_MAXSTRIPS, _lib.RAE_ETK_QCHUNK, _lib.RAE_RK_ROWCHUNK,
            _lib.RAE_ETK_MAXTOP) == (TE, MAXSTRIPS, QROUND, ROWCHUNK, 32)


# ---------------------------------------------------------------------------------- 1. exact
def _exact_inputs(g, nq, n, embed, pad):
    """Small integers: |<Q, A>| <= 9 * 1024, every sum exact in fp32.  A has duplicated rows (with
    their Ab), so equal scores are frequent; the columns of Q past embed are poison."""
    base = g.randint(-3, 4, size=(max(1, n // 3), embed))
    bab = g.randint(-5, 6, size=base.shape[0])
    pick = g.randint(0, base.shape[0], size=n)
    A, Ab = base[pick].astype(np.float32), bab[pick].astype(np.float32)
    Q = np.full((nq, embed + pad), 1000.0, np.float32)          # columns past embed: never read
    Q[:, :embed] = g.randint(-3, 4, size=(nq, embed))
    add = g.randint(-5, 6, size=nq).astype(np.float32)
    # the first and last entity, the tile seams (out of range when n is smaller), out of range
    seams = [0, n - 1, 31, 32, 63, 64, 127, 128, -1, n, 2 ** 31 - 1, -2 ** 31]
    skip = np.array([seams[i % len(seams)] for i in range(nq)], np.int64).astype(np.int32)
    return Q, A, add, Ab, skip


def _product64(Q, A, add, Ab):
    g = Q.astype(np.float64) @ A.astype(np.float64).T
    if add is not None:
        g = g + add.astype(np.float64)[:, None]
    if Ab is not None:
        g = g + Ab.astype(np.float64)[None, :]
    return g


def _ties_across_cut(g, top, skip):
    """Queries whose top-th and (top + 1)-th candidate scores are equal."""
    gm = np.array(g, copy=True)
    n = gm.shape[1]
    if skip is not None:
        sk = skip.astype(np.int64)
        ok = (sk >= 0) & (sk < n)
        gm[np.nonzero(ok)[0], sk[ok]] = -np.inf
    if n <= top:
        return 0
    srt = -np.sort(-gm, axis=1)
    return int(((srt[:, top - 1] == srt[:, top]) & np.isfinite(srt[:, top])).sum())


@pytest.mark.parametrize("embed", [1, 13, 16, 200, 1024])
def test_exact_topk(built_lib, cuda_dev, embed):
    from rae.evaluation import topk_from_scores
    g = np.random.RandomState(300 + embed)
    pad = 4 - embed % 4 if embed % 4 else 4                     # ldq > embed, ldq % 4 == 0
    shapes = [(n, nq) for n in EXACT_N for nq in EXACT_NQ]
    if embed == 16:
        shapes.append((STRIP_SEAM_N, 17))
    ties = 0
    for n, nq in shapes:
        Q, A, add, Ab, skip = _exact_inputs(g, nq, n, embed, pad)
        variants = [(add, Ab, skip)]
        if nq == 130:
            variants += [(None, None, None), (None, Ab, skip), (add, None, None)]
        for ad, ab, sk in variants:
            g64 = _product64(Q[:, :embed], A, ad, ab)
            for top in TOPS:
                ents, scores = topk_queries(built_lib, cuda_dev, Q, A, top, ad, ab, sk,
                                            embed=embed)
                we, ws = topk_from_scores(g64, top, sk)
                assert ents.shape == (nq, top) and scores.shape == (nq, top)
                assert np.array_equal(ents, we), \
                    (embed, n, nq, top, ad is None, ab is None, sk is None,
                     np.nonzero((ents != we).any(axis=1))[0][:8])
                assert np.array_equal(scores.astype(np.float64), ws), (embed, n, nq, top)
                ties += _ties_across_cut(g64, top, sk)
    assert ties > 0                                              # the tie rule was exercised


def test_exact_nan_and_negative_zero(built_lib, cuda_dev):
    """One A row holds an inf and a -inf (its score is NaN or +-inf), one is zero with a zero
    bias, and the queries' add is -0.0: NaN is no candidate, the zero score comes back as +0.0."""
    from rae.evaluation import topk_from_scores
    g = np.random.RandomState(77)
    n, nq, embed = 70, 40, 16
    Q, A, add, Ab, skip = _exact_inputs(g, nq, n, embed, 4)
    skip[:] = -1
    Q[:, :2] = np.where(Q[:, :2] == 0, 1.0, Q[:, :2])           # no 0 * inf
    Q[::5, 1] = -Q[::5, 0]                                       # opposite signs: +-inf, not NaN
    A[33, 0], A[33, 1] = np.inf, -np.inf
    A[40], Ab[40] = 0.0, -0.0
    add[:] = -0.0
    add[1::2] = g.randint(-5, 6, size=add[1::2].shape)
    g64 = _product64(Q[:, :embed], np.where(np.isfinite(A), A, 0.0), add, Ab)
    with np.errstate(invalid="ignore"):
        x = Q[:, 0].astype(np.float64) * A[33, 0] + Q[:, 1].astype(np.float64) * A[33, 1]
        g64[:, 33] = x + g64[:, 33]                               # inf, -inf or NaN
    assert np.isnan(g64[:, 33]).any() and np.isposinf(g64[:, 33]).any() \
        and np.isneginf(g64[:, 33]).any()
    assert (g64[::2, 40] == 0).all()
    for top in (5, 32):
        ents, scores = topk_queries(built_lib, cuda_dev, Q, A, top, add, Ab, skip, embed=embed)
        we, ws = topk_from_scores(g64, top, skip)
        assert np.array_equal(ents, we), np.nonzero((ents != we).any(axis=1))[0][:8]
        assert np.array_equal(scores.astype(np.float64), ws)
        assert not np.isnan(scores).any()
        assert not np.signbit(scores[scores == 0]).any()
    # 32 entities, top = 32: the NaN entity (now 13) is absent exactly from the rows where it is
    # NaN, which then end in padding
    e32, _ = topk_queries(built_lib, cuda_dev, Q, A[20:52], 32, add, Ab[20:52], skip, embed=embed)
    nan_rows = np.isnan(g64[:, 33])
    assert ((e32[nan_rows] == 13).sum(axis=1) == 0).all() and (e32[nan_rows, 31] == -1).all()
    assert ((e32[~nan_rows] == 13).sum(axis=1) == 1).all()


# --------------------------------------------------------------------------- 2. independence
_REAL = {}


def _real_inputs():
    """n = 300, nq = 130, r = 200, real-valued, one duplicated A row; built once."""
    if not _REAL:
        g = np.random.RandomState(21)
        n, nq, r = 300, 130, 200
        Q = g.standard_normal((nq, r)).astype(np.float32)
        A = (g.standard_normal((n, r)) * 0.3).astype(np.float32)
        A[17] = A[200]                                           # a real-valued tie
        add = g.standard_normal(nq).astype(np.float32)
        Ab = g.standard_normal(n).astype(np.float32)
        Ab[17] = Ab[200] = 4.0                                   # ... that is often near the top
        skip = g.randint(0, n, size=nq).astype(np.int32)
        _REAL.update(Q=Q, A=A, add=add, Ab=Ab, skip=skip, g=g)
    return _REAL


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_rows_do_not_depend_on_slot_count_or_order(built_lib, cuda_dev):
    d = _real_inputs()
    Q, A, add, Ab, skip, g = d["Q"], d["A"], d["add"], d["Ab"], d["skip"], d["g"]
    n, nq, top = A.shape[0], Q.shape[0], 10
    run = lambda Q_, a_, s_, A_=A, Ab_=Ab, **kw: topk_queries(built_lib, cuda_dev, Q_, A_, top,
                                                              a_, Ab_, s_, **kw)
    ref = run(Q, add, skip)
    d["out"] = ref
    assert (ref[0] >= 0).all() and np.isfinite(ref[1]).all()
    assert (ref[0] != skip[:, None]).all()
    assert _same(run(Q, add, skip), ref)                         # two runs
    p = g.permutation(nq)                                        # a permutation of the queries
    assert _same(run(Q[p], add[p], skip[p]), (ref[0][p], ref[1][p]))
    extra = g.standard_normal((77, Q.shape[1])).astype(np.float32)
    Qp = np.concatenate([extra[:30], Q, extra[30:]])             # other queries before and after
    pad1 = lambda x, fill: np.concatenate([np.full(30, fill, x.dtype), x, np.full(47, fill, x.dtype)])
    big = run(Qp, pad1(add, 1), pad1(skip, 3))
    assert _same((big[0][30:30 + nq], big[1][30:30 + nq]), ref)
    assert _same(run(Q[40:90], add[40:90], skip[40:90]), (ref[0][40:90], ref[1][40:90]))
    # without scores_out the entities are the same
    e_only, none = run(Q, add, skip, scores=False)
    assert none is None and np.array_equal(e_only, ref[0])
    # a permutation of the entities, skip remapped: the score rows are the same bits, and the
    # entities map back wherever a row has no duplicated score
    pe = g.permutation(n)                        # new entity j is old entity pe[j]
    inv = np.empty(n, np.int64)
    inv[pe] = np.arange(n)
    ep, sp_ = run(Q, add, inv[skip].astype(np.int32), A[pe], Ab[pe])
    assert np.array_equal(bits(sp_), bits(ref[1]))
    distinct = np.array([len(set(row.tolist())) == top for row in bits(ref[1])])
    assert distinct.sum() >= nq // 2 and not distinct.all()      # both kinds of row occur
    assert np.array_equal(pe[ep[distinct]], ref[0][distinct])


def test_query_round_seam(built_lib, cuda_dev):
    """nq = 1024 + 17: two launch rounds; every copy of a query gets the first copy's row."""
    d = _real_inputs()
    Q, A, add, Ab, skip = d["Q"], d["A"], d["add"], d["Ab"], d["skip"]
    top, base = 10, Q.shape[0]
    ref = topk_queries(built_lib, cuda_dev, Q, A, top, add, Ab, skip)
    reps = -(-(QROUND + 17) // base)
    tile = lambda x: np.concatenate([x] * reps)[:QROUND + 17]
    out = topk_queries(built_lib, cuda_dev, tile(Q), A, top, tile(add), Ab, tile(skip))
    assert _same(out, (tile(ref[0]), tile(ref[1])))


# ------------------------------------------------------- 3. the rank kernel's score bits
def test_scores_are_the_rank_kernels(built_lib, cuda_dev):
    """Every returned score, given to rae_rank_queries as the target of its query, is met by an
    entity (equal >= 1) and has exactly its row's strictly better entries above it."""
    d = _real_inputs()
    Q, A, add, Ab, skip = d["Q"], d["A"], d["add"], d["Ab"], d["skip"]
    top, nq = 10, Q.shape[0]
    ents, scores = topk_queries(built_lib, cuda_dev, Q, A, top, add, Ab, skip)
    rep = lambda x: np.repeat(x, top, axis=0)
    gr, eq, _ = rank_queries(built_lib, cuda_dev, rep(Q), A, scores.reshape(-1), rep(add), Ab,
                             rep(skip), lse=False)
    gr, eq = gr.reshape(nq, top), eq.reshape(nq, top)
    assert (eq >= 1).all(), np.argwhere(eq < 1)[:8]
    before = np.array([[int((scores[q, :j] == scores[q, j]).sum()) for j in range(top)]
                       for q in range(nq)])
    assert np.array_equal(gr + before, np.tile(np.arange(top), (nq, 1))), \
        np.argwhere(gr + before != np.arange(top)[None, :])[:8]
    assert (eq >= 2).any()                                       # the duplicated row was returned


# ----------------------------------------------------------------------------------- 4. splits
def _lens(g, N):
    lens = g.randint(1, 12, size=N)
    lens[[0, 5, N - 1]] = 0                                     # empty rows
    return lens


SPLIT_CASES = [
    dict(dec="sp", m=7, r=13, n=257),
    dict(dec="sp", m=100, r=200, n=300),
    dict(dec="rescal", m=7, r=13, n=300),
    dict(dec="rescal", m=7, r=16, n=1000),
    dict(dec="rescal+sp", m=7, r=13, n=500),
    dict(dec="rescal+sp", m=7, r=40, n=257),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: f"{c['dec']}-m{c['m']}-r{c['r']}-n{c['n']}")
def test_split_topk_against_float64(built_lib, cuda_dev, case):
    g = np.random.RandomState(5)
    N, top = 150, 10
    prob = EvalProblem(case["dec"], case["m"], case["r"], 2, _lens(g, N), n=case["n"], seed=3)
    q, c, _, true = queries64(prob.dec, prob.p64, prob.X, prob.a1, prob.a2)
    g64 = scores64(q, c, prob.p64["A"], prob.p64["Ab"]).reshape(2 * N, case["n"])
    skips = {0: None, 1: true.reshape(2 * N)}
    for st in (0, 1):                                            # on the reference, first
        assert_band_cap(g64, top, skips[st], f"{case} skip_true {st}")
    dt = DeviceTopk(DeviceEval(built_lib, prob, cuda_dev))
    for st in (0, 1):
        what = f"{case} skip_true {st}"
        ents, scores = dt.run(0, N, top, st)
        check_topk_against_float64(ents.reshape(2 * N, top), scores.reshape(2 * N, top), g64, top,
                                   skips[st], what)
        # a sub-range: the same bits as the whole split's rows
        pe, ps = dt.run(37, 50, top, st)
        assert np.array_equal(pe, ents[37:87]) and np.array_equal(bits(ps), bits(scores[37:87])), what
        # without scores
        qe, none = dt.run(0, N, top, st, scores=False)
        assert none is None and np.array_equal(qe, ents)
    # nrows == 0 writes nothing; top = 1 and top = 32 are prefixes / extensions of top = 10
    e0, s0 = dt.run(11, 0, top, 0)
    assert e0.shape == (0, 2, top)
    e1, s1 = dt.run(0, N, 1, 1)
    e32, s32 = dt.run(0, N, 32, 1)
    e10, s10 = dt.run(0, N, top, 1)
    assert np.array_equal(e1, e10[:, :, :1]) and np.array_equal(bits(s1), bits(s10[:, :, :1]))
    assert np.array_equal(e32[:, :, :top], e10) and np.array_equal(bits(s32[:, :, :top]), bits(s10))


@pytest.mark.parametrize("dec", ["sp", "rescal", "rescal+sp"])
def test_rows_across_the_row_round_seam(built_lib, cuda_dev, dec):
    """A problem of 2048 + 3 rows: its last six rows straddle the two launch rounds and equal
    the same rows run alone, bitwise."""
    g = np.random.RandomState(9)
    N, top = ROWCHUNK + 3, 5
    prob = EvalProblem(dec, 4, 5, 2, _lens(g, N), n=257, d=60, seed=8)
    dt = DeviceTopk(DeviceEval(built_lib, prob, cuda_dev))
    for st in (0, 1):
        ents, scores = dt.run(0, N, top, st)
        te, ts = dt.run(ROWCHUNK - 3, 6, top, st)
        assert np.array_equal(te, ents[ROWCHUNK - 3:]), (dec, st)
        assert np.array_equal(bits(ts), bits(scores[ROWCHUNK - 3:])), (dec, st)
        assert (ents >= 0).all() and np.isfinite(scores).all()


# ------------------------------------------------------------------------------- 5. the engine
def _trained(dev, dec):
    import torch
    from rae.data import synthetic_dataset
    data, gold = synthetic_dataset(400, 300, 4, seed=31)
    ind = _inducer(data, gold, dev, dec, 8, 16, 4, 50, epochs=1)
    ind.learn(verbose=False)
    torch.cuda.synchronize()
    return data, ind


def _snap(ind):
    eng = ind.engine
    return ([v.detach().clone() for v in ind.modelFunc.named_params().values()],
            [v.detach().clone() for v in ind.optimizer.accumulator],
            int(eng.lib.rae_cursor_moves(eng.plan)), ind.rng.get_state())


def _unchanged(s0, s1):
    import torch
    return all(torch.equal(x, y) for x, y in zip(s0[0], s1[0])) and \
        all(torch.equal(x, y) for x, y in zip(s0[1], s1[1])) and s0[2] == s1[2] and \
        s0[3][2] == s1[3][2] and np.array_equal(s0[3][1], s1[3][1])


def test_engine_relation_preferences(built_lib, cuda_dev):
    import torch
    data, ind = _trained(cuda_dev, "sp")
    eng = ind.engine
    m, top = 8, 6
    s0 = _snap(ind)
    ents, scores = eng.relation_preferences(top)
    torch.cuda.synchronize()
    assert ents.shape == (2, m, top) and ents.dtype == torch.int32 and scores.dtype == torch.float32
    named = ind.modelFunc.named_params()
    p64 = _params(ind)
    # the case whose leniency is capped is the call: its 2 m queries (one ambiguous query of a
    # slot's 8 would already be 12.5 %)
    g64 = np.concatenate([p64[name].T @ p64["A"].T + p64["Ab"][None, :] for name in ("C1", "C2")])
    assert_band_cap(g64, top, None, "preferences")
    for t, name in enumerate(("C1", "C2")):
        he, hs = eng.topk_entities(named[name].detach().t().contiguous(), top)
        assert torch.equal(he, ents[t]) and torch.equal(hs.view(torch.int32), scores[t].view(torch.int32))
        check_topk_against_float64(ents[t].cpu().numpy(), scores[t].cpu().numpy(),
                                   g64[t * m:(t + 1) * m], top, None, f"preferences slot {t + 1}")
    # topk_entities takes host arrays, add and skip
    Qh = p64["C1"].T.astype(np.float32)
    he, hs = eng.topk_entities(Qh, top, add=np.zeros(m, np.float32),
                               skip=np.full(m, -1, np.int32))
    assert torch.equal(he, ents[0])
    sk = ents[0][:, 0].clone()
    he2, _ = eng.topk_entities(Qh, top - 1, skip=sk)
    assert torch.equal(he2, ents[0][:, 1:])                      # the best one left out
    with pytest.raises(ValueError):
        eng.relation_preferences(0)
    with pytest.raises(ValueError):
        eng.topk_entities(Qh, 33)
    assert _unchanged(s0, _snap(ind))


def test_engine_relation_preferences_needs_sp(built_lib, cuda_dev):
    _, ind = _trained(cuda_dev, "rescal")
    with pytest.raises(ValueError):
        ind.engine.relation_preferences(3)


@pytest.mark.parametrize("dec", ["sp", "rescal+sp"])
def test_engine_predict_arguments(built_lib, cuda_dev, dec):
    import torch
    from rae import _lib
    data, ind = _trained(cuda_dev, dec)
    eng, sp_ = ind.engine, ind.engine.split
    s0 = _snap(ind)
    row0, nrows, top = 3, 150, 7
    for st in (False, True):
        ents, scores = eng.predict_arguments(sp_, row0, nrows, top=top, skip_true=st)
        torch.cuda.synchronize()
        assert ents.shape == (nrows, 2, top)
        # a direct rae_eval_topk call with the engine's tensors
        named = ind.modelFunc.named_params()
        p = _lib.ptr
        a = _lib.RaeEvalArgs()
        a.decoder, a.relations, a.embed = _lib.RAE_DEC[dec], 8, 16
        a.n_entities, a.alpha = data.get_arg_voc_size(), 1.0
        a.W, a.Wb, a.A, a.Ab = p(named["W"]), p(named["Wb"]), p(named["A"]), p(named["Ab"])
        a.C1, a.C2, a.R3 = p(named.get("C1")), p(named.get("C2")), p(named.get("R", named.get("C")))
        a.indptr, a.indices, a.values = p(sp_.indptr), p(sp_.indices), p(sp_.values)
        a.args1, a.args2 = p(sp_.args1), p(sp_.args2)
        a.row0, a.nrows = row0, nrows
        need = int(built_lib.rae_topk_workspace_bytes(None, C.byref(a), top))
        ws = torch.empty(need, dtype=torch.uint8, device=cuda_dev)
        a.workspace, a.workspace_bytes = p(ws), need
        de = torch.full((nrows, 2, top), -7, dtype=torch.int32, device=cuda_dev)
        ds = torch.full((nrows, 2, top), float("nan"), dtype=torch.float32, device=cuda_dev)
        o = _lib.RaeTopkOut()
        o.ents, o.scores, o.top, o.skip_true = p(de), p(ds), top, int(st)
        _lib.check(built_lib.rae_eval_topk(C.byref(a), C.byref(o), None), "rae_eval_topk")
        torch.cuda.synchronize()
        assert torch.equal(de, ents) and torch.equal(ds.view(torch.int32), scores.view(torch.int32))
        true = torch.stack([sp_.args1[row0:row0 + nrows], sp_.args2[row0:row0 + nrows]], dim=1)
        hit = (ents == true[:, :, None].to(ents.dtype)).any(dim=2)
        assert not hit.any() if st else hit.any()
        # against the float64 restatement at the engine's parameters
        split = data.split["train"]
        rows = slice(row0, row0 + nrows)
        q, c, _, tr = queries64(dec, _params(ind), split.xFeats[rows], split.args1[rows],
                                split.args2[rows])
        p64 = _params(ind)
        g64 = scores64(q, c, p64["A"], p64["Ab"]).reshape(2 * nrows, -1)
        check_topk_against_float64(ents.cpu().numpy().reshape(2 * nrows, top),
                                   scores.cpu().numpy().reshape(2 * nrows, top), g64, top,
                                   tr.reshape(-1) if st else None, f"predict {dec} skip_true {st}")
    assert eng.predict_arguments(sp_, 7, 0)[0].shape == (0, 2, 10)
    with pytest.raises(IndexError):
        eng.predict_arguments(sp_, 390, 20)
    assert _unchanged(s0, _snap(ind))


def test_cli_prints_parsable_preferences(built_lib, cuda_dev, tmp_path, capsys):
    """python -m rae on the sample with --print-preferences 3 --predict-arguments 4: 2 m lines
    per evaluation whose strings give the device result back."""
    import torch
    from _profile_sample import SAMPLE
    from rae import cli
    from rae import preprocess as P
    plain, out = str(tmp_path / "data-sample.txt"), str(tmp_path / "ds.json.gz")
    with gzip.open(SAMPLE, "rb") as src, open(plain, "wb") as dst:
        shutil.copyfileobj(src, dst)
    P.preprocess(plain, out)
    capsys.readouterr()
    m, epochs, top = 6, 2, 3
    ind = cli.main([out, "--model-name", "m", "--decoder", "sp", "--relations", str(m), "--epochs",
                    str(epochs), "--embed-size", "10", "--neg-samples", "5", "--batch-size", "50",
                    "--print-preferences", str(top), "--predict-arguments", "4",
                    "--predict-top", "2"])
    torch.cuda.synchronize()
    text = capsys.readouterr().out
    pref = [ln for ln in text.splitlines() if ln.startswith("preferences\t")]
    assert len(pref) == epochs * 2 * m, text
    ents, scores = ind.engine.relation_preferences(top)
    ents, scores = ents.cpu().numpy(), scores.cpu().numpy()
    arg2id = ind.data.arg2Id
    assert any(not name.isdigit() for name in arg2id)            # strings, not ids
    last = pref[-2 * m:]                                         # the final parameters'
    for i, ln in enumerate(last):
        f = ln.split("\t")
        k, t = i // 2, i % 2
        assert (f[1], f[2]) == (str(k), str(t + 1))
        pairs = [x.rsplit(":", 1) for x in f[3:]]
        assert len(pairs) == top
        assert [arg2id[name] for name, _ in pairs] == ents[t, k].tolist()
        got = np.array([float(v) for _, v in pairs], dtype=np.float32)
        assert np.array_equal(bits(got), bits(scores[t, k]))
    pred = [ln for ln in text.splitlines() if ln.startswith("predictions\t")]
    assert len(pred) == 4 * 2 and text.count(" predictions (4 rows)") == 1
    pe, ps = ind.engine.predict_arguments(ind.engine.split, 0, 4, top=2)
    first = pred[0].split("\t")
    id2arg = ind.data.id2Arg
    assert first[1:4] == ["0", "1", id2arg[int(ind.data.split["train"].args1[0])]]
    assert [arg2id[x.rsplit(":", 1)[0]] for x in first[4:]] == pe[0, 0].cpu().tolist()
