"""Argument ranking over the whole entity vocabulary (rae_rank_queries, rae_eval_rank,
TrainEngine.rank, --eval-rank) on an MI355X.

References: exact integer counts in numpy for rae_rank_queries on small-integer inputs (every
fp32 operation is exact there); the float64 restatement of tests/_rank_ref.py (pinned to the
oracle by tests/test_rank_host.py) for rae_eval_rank, compared through intervals: with
tol = TERM_ATOL + TERM_RTOL max(|u|, |g|) (test_gpu_eval's tolerances, in score space),
lo = #{g > u + tol} <= greater and greater + equal <= hi = #{g > u - tol}.  The leniency is capped
on the reference alone: at most 10 % of a case's queries with hi > lo, no interval wider than 4.
"""
import numpy as np
import pytest

from _entry_ref import DeviceEval, EvalProblem
from _rank_ref import (DeviceRank, assert_cap, counts_exact, intervals, lse64, queries64,
                       rank_queries, scores64)
from test_gpu_eval import TERM_ATOL, TERM_RTOL, _inducer, _params

pytestmark = pytest.mark.gpu

# the kernel's seams (csrc/rae_rank.hpp): a 32 x 32 MFMA tile, 64 entities per wave, RAE_RK_TE =
# 128 entities per tile = one strip up to 128 tiles; beyond 128 * 128 entities a strip takes two
TE, MAXSTRIPS, QCHUNK, ROWCHUNK = 128, 128, 4096, 2048
EXACT_N = [1, 15, 17, 31, 32, 33, 64, 65, 127, 128, 129, 257, 385]
STRIP_SEAM_N = TE * MAXSTRIPS + 1          # 129 tiles: two tiles per strip, the last strip short
EXACT_NQ = [0, 1, 17, 130]


def test_constants_are_the_kernels():
    from rae import _lib
    assert (_lib.RAE_RK_TE, _lib.RAE_RK_MAXSTRIPS, _lib.RAE_RK_QCHUNK, _lib.RAE_RK_ROWCHUNK) == \
        (TE, MAXSTRIPS, QCHUNK, ROWCHUNK)


# ---------------------------------------------------------------------------------- 1. exact
def _exact_inputs(g, nq, n, embed, pad):
    """Small integers: |<Q, A>| <= 9 * 1024, every sum exact in fp32.  A has duplicated rows (with
    their Ab) and the targets are scores of existing entities, so that g == target happens."""
    base = g.randint(-3, 4, size=(max(1, n // 3), embed))
    bab = g.randint(-5, 6, size=base.shape[0])
    pick = g.randint(0, base.shape[0], size=n)
    A, Ab = base[pick].astype(np.float32), bab[pick].astype(np.float32)
    Q = np.full((nq, embed + pad), 1000.0, np.float32)          # columns past embed: never read
    Q[:, :embed] = g.randint(-3, 4, size=(nq, embed))
    add = g.randint(-5, 6, size=nq).astype(np.float32)
    e_star = g.randint(0, n, size=nq)
    target = (Q[:, :embed].astype(np.float64) * A[e_star]).sum(axis=1) + add + Ab[e_star]
    target = (target + g.randint(0, 2, size=nq) * g.randint(-2, 3, size=nq)).astype(np.float32)
    # the first and last entity, the tile seams (out of range when n is smaller), out of range
    seams = [0, n - 1, 31, 32, 63, 64, 127, 128, -1, n, n + 5, 2 ** 31 - 1, -2 ** 31]
    skip = np.array([seams[i % len(seams)] for i in range(nq)], np.int64).astype(np.int32)
    return Q, A, add, Ab, target, skip


@pytest.mark.parametrize("embed", [1, 13, 16, 200, 1024])
def test_exact_counts(built_lib, cuda_dev, embed):
    g = np.random.RandomState(100 + embed)
    pad = 4 - embed % 4 if embed % 4 else 4                     # ldq > embed, ldq % 4 == 0
    shapes = [(n, nq) for n in EXACT_N for nq in EXACT_NQ] + [(STRIP_SEAM_N, 17)]
    ties = 0
    for n, nq in shapes:
        Q, A, add, Ab, target, skip = _exact_inputs(g, nq, n, embed, pad)
        variants = [(add, Ab, skip)]
        if nq == 130:
            variants += [(None, None, None), (None, Ab, skip), (add, None, None)]
        for ad, ab, sk in variants:
            t = target
            gr, eq, _ = rank_queries(built_lib, cuda_dev, Q, A, t, ad, ab, sk, embed=embed,
                                     lse=False)
            wg, we = counts_exact(Q[:, :embed], A, ad, ab, t, sk)
            assert np.array_equal(gr, wg) and np.array_equal(eq, we), \
                (embed, n, nq, ad is None, ab is None, sk is None,
                 np.nonzero((gr != wg) | (eq != we))[0][:8])
            ties += int(we.sum())
    assert ties > 0                                              # the == path was exercised


def test_exact_counts_do_not_depend_on_lse(built_lib, cuda_dev):
    """The counting epilogue is one code path with and without the log-sum-exp."""
    g = np.random.RandomState(7)
    Q, A, add, Ab, target, skip = _exact_inputs(g, 130, 385, 16, 4)
    a = rank_queries(built_lib, cuda_dev, Q, A, target, add, Ab, skip, embed=16, lse=False)
    b = rank_queries(built_lib, cuda_dev, Q, A, target, add, Ab, skip, embed=16, lse=True)
    wg, we = counts_exact(Q[:, :16], A, add, Ab, target, skip)
    assert np.array_equal(a[0], wg) and np.array_equal(a[1], we)
    assert np.array_equal(b[0], wg) and np.array_equal(b[1], we)


# --------------------------------------------------------------------------- 2. independence
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_outputs_do_not_depend_on_slot_count_or_order(built_lib, cuda_dev):
    g = np.random.RandomState(21)
    n, nq, r = 300, 130, 200
    Q = g.standard_normal((nq, r)).astype(np.float32)
    A = (g.standard_normal((n, r)) * 0.3).astype(np.float32)
    A[17] = A[200]                                               # a real-valued tie candidate
    add = g.standard_normal(nq).astype(np.float32)
    Ab = g.standard_normal(n).astype(np.float32)
    Ab[17] = Ab[200]
    skip = g.randint(0, n, size=nq).astype(np.int32)
    target = (g.standard_normal(nq) * 3).astype(np.float32)
    run = lambda Q_, t_, a_, s_, A_=A, Ab_=Ab: rank_queries(built_lib, cuda_dev, Q_, A_, t_, a_,
                                                            Ab_, s_)
    gr, eq, ls = run(Q, target, add, skip)
    assert np.isfinite(ls).all() and gr.min() >= 0 and (gr + eq).max() <= n - 1
    # two runs: bitwise, lse included
    gr2, eq2, ls2 = run(Q, target, add, skip)
    assert np.array_equal(gr, gr2) and np.array_equal(eq, eq2)
    assert np.array_equal(_bits(ls), _bits(ls2))
    # a permutation of the queries
    p = g.permutation(nq)
    grp, eqp, lsp = run(Q[p], target[p], add[p], skip[p])
    assert np.array_equal(grp, gr[p]) and np.array_equal(eqp, eq[p])
    assert np.array_equal(_bits(lsp), _bits(ls[p]))
    # padding nq (other queries after and before), and a sub-range
    extra = g.standard_normal((77, r)).astype(np.float32)
    Qp = np.concatenate([extra[:30], Q, extra[30:]])
    pad1 = lambda x, fill: np.concatenate([np.full(30, fill, x.dtype), x, np.full(47, fill, x.dtype)])
    grq, eqq, lsq = run(Qp, pad1(target, 0), pad1(add, 1), pad1(skip, 3))
    assert np.array_equal(grq[30:30 + nq], gr) and np.array_equal(eqq[30:30 + nq], eq)
    assert np.array_equal(_bits(lsq[30:30 + nq]), _bits(ls))
    grs, eqs, lss = run(Q[40:90], target[40:90], add[40:90], skip[40:90])
    assert np.array_equal(grs, gr[40:90]) and np.array_equal(eqs, eq[40:90])
    assert np.array_equal(_bits(lss), _bits(ls[40:90]))
    # a permutation of the entities, skip remapped: the counts are unchanged
    pe = g.permutation(n)                        # new entity j is old entity pe[j]
    inv = np.empty(n, np.int64)
    inv[pe] = np.arange(n)
    gre, eqe, _ = run(Q, target, add, inv[skip].astype(np.int32), A[pe], Ab[pe])
    assert np.array_equal(gre, gr) and np.array_equal(eqe, eq)


def test_query_chunk_seam(built_lib, cuda_dev):
    """nq = 4096 + 17: two launch rounds; every copy of a query gets the first copy's bits."""
    g = np.random.RandomState(22)
    n, r, base = 300, 16, 130
    reps = -(-(QCHUNK + 17) // base)
    Q = g.standard_normal((base, r)).astype(np.float32)
    A = g.standard_normal((n, r)).astype(np.float32)
    Ab = g.standard_normal(n).astype(np.float32)
    target = g.standard_normal(base).astype(np.float32)
    skip = g.randint(0, n, size=base).astype(np.int32)
    gr, eq, ls = rank_queries(built_lib, cuda_dev, Q, A, target, None, Ab, skip)
    tile = lambda x: np.concatenate([x] * reps)[:QCHUNK + 17]
    grt, eqt, lst = rank_queries(built_lib, cuda_dev, tile(Q), A, tile(target), None, Ab, tile(skip))
    assert np.array_equal(grt, tile(gr)) and np.array_equal(eqt, tile(eq))
    assert np.array_equal(_bits(lst), _bits(tile(ls)))


# -------------------------------------------------------------------------------------- 3. lse
@pytest.mark.parametrize("n,r", [(1, 16), (300, 16), (1000, 13), (STRIP_SEAM_N + 300, 16),
                                 (700, 200)])
def test_lse_against_float64(built_lib, cuda_dev, n, r):
    g = np.random.RandomState(n + r)
    nq = 70
    sq = 3.0 if r <= 16 else 1.5
    Q = (g.standard_normal((nq, r)) * sq).astype(np.float32)
    A = (g.standard_normal((n, r)) * sq).astype(np.float32)
    add = (g.standard_normal(nq) * 2).astype(np.float32)
    Ab = (g.standard_normal(n) * 2).astype(np.float32)
    skip = g.randint(0, n, size=nq).astype(np.int32)
    skip[::3] = -1                                               # nothing skipped
    target = np.zeros(nq, np.float32)
    gr, eq, ls = rank_queries(built_lib, cuda_dev, Q, A, target, add, Ab, skip)
    Q64, A64 = Q.astype(np.float64), A.astype(np.float64)
    g64 = Q64 @ A64.T + add.astype(np.float64)[:, None] + Ab.astype(np.float64)[None, :]
    if n > 1:
        spread = g64.max() - g64.min()
        print(f"n {n} r {r}: scores in [{g64.min():.1f}, {g64.max():.1f}]")
        assert spread > 120.0                                    # the rescaling is exercised
    g64x = np.concatenate([g64, np.full((nq, 1), -np.inf)], axis=1)      # column n: nothing
    want = lse64(g64x, np.where(skip >= 0, skip, n).astype(np.int64))
    E = (r + 3) * 2.0 ** -24 * (np.abs(Q64) @ np.abs(A64).T + np.abs(add)[:, None] +
                                np.abs(Ab)[None, :]).max(axis=1)
    if n == 1:
        assert np.array_equal(np.isneginf(ls), skip == 0) and (skip == 0).any()
    assert np.array_equal(np.isneginf(ls), np.isneginf(want))
    fin = np.isfinite(want)
    err = np.abs(ls[fin].astype(np.float64) - want[fin])
    bound = E[fin] + TERM_ATOL + TERM_RTOL * np.abs(want[fin])
    print(f"n {n} r {r}: max |lse - lse64| {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (err.max(), bound.min())


# ----------------------------------------------------------------------------------- 4. splits
def _lens(g, N):
    lens = g.randint(1, 12, size=N)
    lens[[0, 5, N - 1]] = 0                                     # empty rows
    return lens


SPLIT_CASES = [
    dict(dec="sp", m=7, r=13, n=257),
    dict(dec="sp", m=100, r=200, n=300),
    dict(dec="sp", m=7, r=16, n=500),
    dict(dec="rescal", m=7, r=13, n=300),
    dict(dec="rescal", m=7, r=16, n=1000),
    dict(dec="rescal+sp", m=7, r=13, n=500),
    dict(dec="rescal+sp", m=7, r=40, n=257),
]
_REF = {}


def _reference(prob, values=True):
    """(u, true, lo, hi, lse) of every row of the problem in float64, computed once per case."""
    key = (id(prob), values)
    if key not in _REF:
        X = prob.X
        if not values:
            X = X.copy()
            X.data[:] = 1.0
        q, c, u, true = queries64(prob.dec, prob.p64, X, prob.a1, prob.a2)
        g = scores64(q, c, prob.p64["A"], prob.p64["Ab"])
        lo, hi = intervals(g, u, true)
        _REF[key] = (prob, u, true, lo, hi, lse64(g, true))
    return _REF[key][1:]


def _check_ranks(out, ref, row0, nrows, what):
    gr, eq, tg, ls, _ = out
    u, true, lo, hi, l64 = (x[row0:row0 + nrows] for x in ref)
    np.testing.assert_allclose(tg, u, rtol=TERM_RTOL, atol=TERM_ATOL, err_msg=what)
    bad = (gr < lo) | (gr + eq > hi) | (eq < 0)
    print(f"{what}: {int((gr != lo).sum())} of {gr.size} counts differ from the float64 lower end, "
          f"{int(bad.sum())} outside their interval, max |lse - lse64| "
          f"{np.abs(ls - l64).max() if gr.size else 0.0:.3e}")
    assert not bad.any(), (what, np.argwhere(bad)[:8])
    assert np.isfinite(ls).all(), what


def _check_summary(out, ks, what):
    from rae.evaluation import rank_summary
    gr, eq, tg, ls, summ = out
    want = rank_summary(gr, eq, tg, ls, ks)
    for side in range(2):
        for j in (3, 4, 5, 6, 7):
            assert summ[8 * side + j] == want[8 * side + j], (what, side, j)
        for j in (0, 1, 2):
            a, b = summ[8 * side + j], want[8 * side + j]
            assert abs(a - b) <= 1e-12 * abs(b), (what, side, j, a, b)


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: f"{c['dec']}-m{c['m']}-r{c['r']}-n{c['n']}")
def test_split_ranks_against_float64(built_lib, cuda_dev, case):
    g = np.random.RandomState(5)
    N = 200
    prob = EvalProblem(case["dec"], case["m"], case["r"], 2, _lens(g, N), n=case["n"], seed=3)
    assert (prob.a1 == prob.a2).any() and (np.diff(prob.X.indptr) == 0).any()
    what = str(case)
    ref = _reference(prob)
    assert_cap(ref[2], ref[3], what)                       # on the reference, before the device
    dr = DeviceRank(DeviceEval(built_lib, prob, cuda_dev))
    ks = (1, 10, 100)
    whole = dr.run(0, N, ks)
    _check_ranks(whole, ref, 0, N, what)
    _check_summary(whole, ks, what)
    assert whole[4][7] == N and whole[4][15] == N
    # row0 > 0: the same bits as the whole split's rows; its own summary
    part = dr.run(37, 50, ks)
    for a, b in zip(part[:4], whole[:4]):
        assert np.array_equal(a.view(np.uint32), b[37:87].view(np.uint32)), what
    _check_summary(part, ks, what + " rows [37, 87)")
    one = dr.run(N - 1, 1, (3,))
    for a, b in zip(one[:4], whole[:4]):
        assert np.array_equal(a.view(np.uint32), b[N - 1:].view(np.uint32)), what
    _check_summary(one, (3,), what + " last row")
    # without the per-query float outputs the summary is the same (they live in the workspace)
    quiet = dr.run(0, N, ks, per_query=False)
    assert np.array_equal(quiet[4], whole[4]) and np.array_equal(quiet[0], whole[0])
    # nrows == 0: a zero summary, nothing else written
    empty = dr.run(11, 0, ks)
    assert empty[0].shape == (0, 2) and not empty[4].any()
    # values NULL: binary features
    refb = _reference(prob, values=False)
    assert_cap(refb[2], refb[3], what + " binary")
    _check_ranks(dr.run(0, N, ks, values=False), refb, 0, N, what + " binary")


@pytest.mark.parametrize("dec", ["sp", "rescal", "rescal+sp"])
def test_range_across_the_chunk_seam(built_lib, cuda_dev, dec):
    """Rows [5, 5 + 2048 + 17): two launch rounds, the second of 17 rows."""
    g = np.random.RandomState(9)
    N = 5 + ROWCHUNK + 17 + 3
    prob = EvalProblem(dec, 4, 5, 2, _lens(g, N), n=257, d=60, seed=8)
    ref = _reference(prob)
    what = f"{dec} across the chunk seam"
    assert_cap(ref[2], ref[3], what)
    dr = DeviceRank(DeviceEval(built_lib, prob, cuda_dev))
    out = dr.run(5, ROWCHUNK + 17, (1, 10, 100, 200))
    _check_ranks(out, ref, 5, ROWCHUNK + 17, what)
    _check_summary(out, (1, 10, 100, 200), what)
    tail = dr.run(5 + ROWCHUNK - 3, 20, (1,))
    for a, b in zip(tail[:4], out[:4]):
        assert np.array_equal(a.view(np.uint32), b[ROWCHUNK - 3:].view(np.uint32))


# ------------------------------------------------------------- 5. rae_eval_cost is unchanged
@pytest.mark.parametrize("dec", ["sp", "rescal", "rescal+sp"])
def test_eval_cost_bits_survive_a_rank_call_on_its_workspace(built_lib, cuda_dev, dec):
    import torch
    g = np.random.RandomState(2)
    prob = EvalProblem(dec, 12, 20, 3, _lens(g, 120), n=90, seed=6)
    de = DeviceEval(built_lib, prob, cuda_dev)
    dr = DeviceRank(de)                                   # one workspace for both entries
    before, sums0 = de.run(0, 120)
    de.poison()
    dr.run(3, 100)
    after, sums1 = de.run(0, 120)
    assert torch.equal(before, after) and sums0 == sums1
    assert torch.isfinite(before).all()


# ----------------------------------------------------------------------------- 6. the surface
def test_engine_rank_touches_nothing(built_lib, cuda_dev):
    import torch
    from rae.data import synthetic_dataset
    from rae.evaluation import rank_summary
    data, gold = synthetic_dataset(400, 300, 4, seed=31)
    ind = _inducer(data, gold, cuda_dev, "rescal+sp", 8, 16, 4, 50, epochs=1)
    ind.learn(verbose=False)
    torch.cuda.synchronize()
    eng = ind.engine
    snap = lambda: ([v.detach().clone() for v in ind.modelFunc.named_params().values()],
                    [v.detach().clone() for v in ind.optimizer.accumulator],
                    int(eng.lib.rae_cursor_moves(eng.plan)), ind.rng.get_state())
    p0, a0, c0, s0 = snap()
    res = eng.rank(eng.split, 3, 150, ks=(1, 5), per_query=True)
    p1, a1, c1, s1 = snap()
    assert all(torch.equal(x, y) for x, y in zip(p0, p1))
    assert all(torch.equal(x, y) for x, y in zip(a0, a1))
    assert c0 == c1 and s0[2] == s1[2] and np.array_equal(s0[1], s1[1])
    n = data.get_arg_voc_size()
    assert res.nrows == 150 and res.greater.shape == (150, 2) and set(res.hits) == {1, 5}
    want = rank_summary(res.greater.cpu().numpy(), res.equal.cpu().numpy(),
                        res.target.cpu().numpy(), res.lse.cpu().numpy(), (1, 5))
    assert np.allclose(res.summary, want, rtol=1e-12, atol=0)
    for side in range(2):
        assert 1.0 <= res.mean_rank[side] <= n and 0.0 < res.mrr[side] <= 1.0
        assert res.logp[side] < 0.0 and 0.0 <= res.hits[1][side] <= res.hits[5][side] <= 1.0
    assert abs(res.mrr[2] - (res.mrr[0] + res.mrr[1]) / 2) < 1e-15
    again = eng.rank(eng.split, 3, 150, ks=(1, 5))
    assert again.summary == res.summary and again.greater is None
    assert eng.rank(eng.split, 7, 0).summary == (0.0,) * 16
    with pytest.raises(IndexError):
        eng.rank(eng.split, 390, 20)
    # against the float64 restatement at the engine's own parameters
    split = data.split["train"]
    q, c, u, true = queries64("rescal+sp", _params(ind), split.xFeats[3:153], split.args1[3:153],
                              split.args2[3:153])
    p64 = _params(ind)
    lo, hi = intervals(scores64(q, c, p64["A"], p64["Ab"]), u, true)
    gr, eq = res.greater.cpu().numpy(), res.equal.cpu().numpy()
    assert ((gr >= lo) & (gr + eq <= hi)).all()


def test_inducer_fills_rank_metrics(built_lib, cuda_dev, capsys):
    from test_gpu_eval import _three_splits
    data, gold = _three_splits()
    ind = _inducer(data, gold, cuda_dev, "sp", 8, 16, 4, 50, epochs=2, eval_rank=True,
                   eval_rank_ks=(1, 10), eval_rank_rows=120)
    ind.learn(verbose=True)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if " ranking: " in ln]
    assert [ln.split()[0] for ln in lines] == ["valid", "test"] * 2, out
    assert all("MRR" in ln and "hits@10" in ln and "(120 rows)" in ln for ln in lines)
    assert len(ind.rank_metrics["valid"]) == 2 and len(ind.rank_metrics["test"]) == 2
    assert ind.rank_metrics["train"] == []
    assert all(r.nrows == 120 and np.isfinite(r.summary).all() for r in ind.rank_metrics["valid"])
    off = _inducer(data, gold, cuda_dev, "sp", 8, 16, 4, 50, epochs=1)
    off.learn(verbose=True)
    assert " ranking: " not in capsys.readouterr().out and off.rank_metrics["valid"] == []


def test_cli_flags_parse():
    from rae.cli import get_command_args
    base = ["data.npz", "--model-name", "m", "--decoder", "sp"]
    a = get_command_args(base)
    assert a.eval_rank is False and tuple(a.eval_rank_ks) == (1, 10, 100) and a.eval_rank_rows is None
    a = get_command_args(base + ["--eval-rank", "--eval-rank-ks", "1,3,50,1000",
                                 "--eval-rank-rows", "4096"])
    assert a.eval_rank is True and a.eval_rank_ks == (1, 3, 50, 1000) and a.eval_rank_rows == 4096
    for bad in ("1,2,3,4,5", "0,1", "x"):
        with pytest.raises(SystemExit):
            get_command_args(base + ["--eval-rank-ks", bad])
