"""Host-side checks of the argument ranking (no GPU): the float64 restatement of
tests/_rank_ref.py is pinned to the reference-pinned oracle, rank_summary on hand cases, and the
three new entry points reject bad arguments before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import rae_oracle as O
from _entry_ref import EvalProblem
from _rank_ref import DEC_ID, queries64, scores64


def _logsig(x):
    return -np.logaddexp(0.0, -x)


# ------------------------------------------------- 1. the restatement against the oracle
@pytest.mark.parametrize("dec", ["sp", "rescal", "rescal+sp"])
def test_restatement_matches_the_oracle_with_every_entity_as_negative(dec):
    n, l = 37, 23
    prob = EvalProblem(dec, 7, 13, 3, [0, 1, 5] + [4] * (l - 3), n=n, d=120, seed=11)
    neg = np.repeat(np.arange(n, dtype=np.int32)[:, None], l, axis=1)      # neg[t, b] = t
    res = O.train_step_grads(dec, prob.p64, prob.X, prob.a1, prob.a2, neg, neg, alpha=1.0)
    q, c, u, true = queries64(dec, prob.p64, prob.X, prob.a1, prob.a2)
    g = scores64(q, c, prob.p64["A"], prob.p64["Ab"])                      # (l, 2, n)
    assert np.array_equal(true[:, 0], prob.a1) and np.array_equal(true[:, 1], prob.a2)
    # positives: all_scores[:l] = logsig(u_1), [l:2l] = logsig(u_2)
    np.testing.assert_allclose(res.scores[:l], _logsig(u[:, 0]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.scores[l:2 * l], _logsig(u[:, 1]), rtol=0, atol=1e-12)
    negs = res.scores[4 * l:]
    want = _logsig(-g)
    if dec == "sp":                       # (2n, l): side, entity, example
        got = negs.reshape(2, n, l).transpose(2, 0, 1)
    else:                                 # (2, l, n): side, example, entity
        got = negs.reshape(2, l, n).transpose(1, 0, 2)
    err = np.abs(got - want).max()
    print(f"{dec}: max |oracle - restatement| over the negative scores {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # the other decoders' layout of the same vector does not fit: the check tells them apart
    other = negs.reshape(2, l, n).transpose(1, 0, 2) if dec == "sp" else \
        negs.reshape(2, n, l).transpose(2, 0, 1)
    assert np.abs(other - want).max() > 1e-3


# ---------------------------------------------------------------------- 2. rank_summary
def test_rank_summary_hand_cases():
    from rae.evaluation import rank_summary
    # three rows; side 0: ranks 1, 2.5 (a tie pair), 11; side 1: ranks 10, 10.5, 101
    greater = np.array([[0, 9], [1, 9], [10, 100]])
    equal = np.array([[0, 0], [1, 1], [0, 0]])
    target = np.array([[0.5, -1.0], [2.0, 0.0], [-3.0, 1.5]])
    lse = np.array([[0.5, 2.0], [-np.inf, 0.0], [1.0, 1.5]])
    s = rank_summary(greater, equal, target, lse, ks=(1, 10, 100))
    rank = np.array([[1.0, 10.0], [2.5, 10.5], [11.0, 101.0]])
    logp = np.array([[-np.log(2), -1.0 - np.logaddexp(-1.0, 2.0)],
                     [0.0, -np.log(2)],                                  # lse = -inf: logp = 0
                     [-3.0 - np.logaddexp(-3.0, 1.0), -np.log(2)]])
    for side in range(2):
        np.testing.assert_allclose(s[8 * side + 0], (1 / rank[:, side]).sum(), rtol=1e-15)
        assert s[8 * side + 1] == rank[:, side].sum()
        np.testing.assert_allclose(s[8 * side + 2], logp[:, side].sum(), rtol=1e-14)
        assert s[8 * side + 7] == 3.0
    # hits at the boundary: rank == k counts, rank == k + 1/2 does not
    assert list(s[3:7]) == [1.0, 2.0, 3.0, 0.0]              # ranks 1, 2.5, 11
    assert list(s[11:15]) == [0.0, 1.0, 2.0, 0.0]            # ranks 10, 10.5, 101
    # unused thresholds count nothing; the fourth slot is used when given
    s4 = rank_summary(greater, equal, target, lse, ks=(0, 11, -3, 101))
    assert list(s4[3:7]) == [0.0, 3.0, 0.0, 3.0] and list(s4[11:15]) == [0.0, 2.0, 0.0, 3.0]
    with pytest.raises(ValueError):
        rank_summary(greater, equal, target, lse, ks=(1, 2, 3, 4, 5))


def test_rank_summary_single_entity_and_empty():
    from rae.evaluation import rank_summary
    # n == 1: the only entity is the true one, nothing is counted or summed
    s = rank_summary(np.zeros((4, 2)), np.zeros((4, 2)), np.full((4, 2), 0.7),
                     np.full((4, 2), -np.inf), ks=(1,))
    for side in range(2):
        assert s[8 * side + 0] == 4.0 and s[8 * side + 1] == 4.0      # rank 1
        assert s[8 * side + 2] == 0.0                                  # logp 0
        assert s[8 * side + 3] == 4.0 and s[8 * side + 7] == 4.0
    z = rank_summary(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)))
    assert not z.any() and z.shape == (16,)
    # all ties: rank = 1 + equal / 2
    t = rank_summary([[0, 0]], [[4, 1]], [[0.0, 0.0]], [[0.0, 0.0]], ks=(2, 3))
    assert t[1] == 3.0 and t[9] == 1.5 and list(t[3:5]) == [0.0, 1.0] and list(t[11:13]) == [1.0, 1.0]


# -------------------------------------------------------------- 3. rejection without a GPU
_KEEP = []


def _buf(nbytes, align=256, offset=0):
    """A host address with the given alignment (never dereferenced: every case is rejected, or
    is a workspace-bytes query, before a HIP call)."""
    raw = C.create_string_buffer(nbytes + align + 16)
    _KEEP.append(raw)
    base = C.addressof(raw)
    return ((base + align - 1) // align) * align + offset


def _rank_args(lib, **kw):
    from rae import _lib
    a = _lib.RaeRankArgs()
    a.Q, a.ldq, a.nq = _buf(4096), 16, 8
    a.add, a.target, a.skip = _buf(64), _buf(64), _buf(64)
    a.A, a.Ab, a.n_entities, a.embed = _buf(4096), _buf(64), 10, 16
    a.greater, a.equal, a.lse = _buf(64), _buf(64), _buf(64)
    need = lib.rae_rank_workspace_bytes(C.byref(a), None)
    assert need > 0
    a.workspace, a.workspace_bytes = _buf(16), need
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _eval_args(lib, dec="sp", **kw):
    from rae import _lib
    a = _lib.RaeEvalArgs()
    a.decoder, a.relations, a.embed, a.neg_samples = DEC_ID[dec], 8, 16, 0
    a.n_entities, a.alpha = 10, 1.0
    for f in ("W", "Wb", "A", "Ab", "C1", "C2", "R3", "indptr", "indices", "values", "args1",
              "args2"):
        setattr(a, f, _buf(64))
    a.row0, a.nrows = 0, 4
    for k, v in kw.items():
        setattr(a, k, v)
    need = lib.rae_rank_workspace_bytes(None, C.byref(a))
    a.workspace, a.workspace_bytes = _buf(16), max(need, 0)
    return a


def _rank_out(**kw):
    from rae import _lib
    o = _lib.RaeRankOut()
    o.greater, o.equal, o.target, o.lse, o.summary = (_buf(64) for _ in range(5))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


RANK_BAD = [
    dict(Q=None), dict(target=None), dict(A=None), dict(greater=None), dict(equal=None),
    dict(workspace=None),
    dict(embed=0), dict(embed=1025, ldq=1028),
    dict(ldq=12), dict(ldq=18), dict(Q=_buf(4096, 256, 4)), dict(A=_buf(4096, 256, 8)),
    dict(n_entities=0), dict(n_entities=1 << 31), dict(nq=-1),
    dict(workspace_bytes=255), dict(workspace=_buf(4096, 256, 64)),
]


@pytest.mark.parametrize("bad", RANK_BAD, ids=lambda b: "-".join(f"{k}" for k in b))
def test_rank_queries_rejects(built_lib, bad):
    from rae import _lib
    assert _lib.RAE_OK == 0
    a = _rank_args(built_lib)
    if "workspace_bytes" in bad:
        bad = dict(workspace_bytes=a.workspace_bytes - 1)
    for k, v in bad.items():
        setattr(a, k, v)
    assert built_lib.rae_rank_queries(C.byref(a), None) == -1, bad       # RAE_E_INVALID
    assert built_lib.rae_last_error()


def test_rank_queries_rejects_null_struct(built_lib):
    assert built_lib.rae_rank_queries(None, None) == -1
    assert built_lib.rae_eval_rank(None, None, None) == -1


EVAL_BAD = [
    ("sp", dict(W=None)), ("sp", dict(Wb=None)), ("sp", dict(A=None)), ("sp", dict(Ab=None)),
    ("sp", dict(C1=None)), ("rescal+sp", dict(C2=None)), ("rescal", dict(R3=None)),
    ("sp", dict(indptr=None)), ("sp", dict(indices=None)), ("sp", dict(args1=None)),
    ("sp", dict(args2=None)), ("sp", dict(workspace=None)),
    ("sp", dict(embed=0)), ("sp", dict(embed=1025)),
    ("sp", dict(n_entities=0)), ("sp", dict(n_entities=1 << 31)),
    ("sp", dict(nrows=-1)), ("sp", dict(row0=-1)), ("sp", dict(decoder=3)),
    ("sp", dict(relations=0)), ("sp", dict(relations=130)),
    ("rescal", dict(relations=324)), ("rescal+sp", dict(relations=324)),   # bilinear limit: 320
    ("sp", dict(A=_buf(64, 256, 4))), ("sp", dict(W=_buf(64, 256, 4))),
]


@pytest.mark.parametrize("dec,bad", EVAL_BAD, ids=lambda b: "-".join(b) if isinstance(b, dict) else b)
def test_eval_rank_rejects(built_lib, dec, bad):
    a = _eval_args(built_lib, dec)
    for k, v in bad.items():
        setattr(a, k, v)
    assert built_lib.rae_eval_rank(C.byref(a), C.byref(_rank_out()), None) == -1, (dec, bad)
    assert built_lib.rae_last_error()


def test_eval_rank_rejects_outputs_and_workspace(built_lib):
    lib = built_lib
    a = _eval_args(lib)
    assert lib.rae_eval_rank(C.byref(a), None, None) == -1
    assert lib.rae_eval_rank(C.byref(a), C.byref(_rank_out(greater=None)), None) == -1
    assert lib.rae_eval_rank(C.byref(a), C.byref(_rank_out(equal=None)), None) == -1
    short = _eval_args(lib)
    short.workspace_bytes -= 1
    assert lib.rae_eval_rank(C.byref(short), C.byref(_rank_out()), None) == -1
    assert b"workspace_bytes" in lib.rae_last_error()
    mis = _eval_args(lib)
    mis.workspace = _buf(4096, 256, 128)
    assert lib.rae_eval_rank(C.byref(mis), C.byref(_rank_out()), None) == -1
    assert b"256-byte" in lib.rae_last_error()
    # the bilinear relations limit binds the bilinear decoders only
    assert lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, "sp", relations=324))) > 0
    assert lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, "rescal", relations=320))) > 0


# ------------------------------------------------------------------- 4. workspace bytes
def test_workspace_bytes_without_a_gpu(built_lib):
    from rae import _lib
    lib = built_lib
    assert lib.rae_rank_workspace_bytes(None, None) == -1
    a, e = _rank_args(lib), _eval_args(lib)
    assert lib.rae_rank_workspace_bytes(C.byref(a), C.byref(e)) == -1
    # independent of nq / nrows, of the pointers, and of n_entities beyond the strip count
    base = lib.rae_rank_workspace_bytes(C.byref(a), None)
    for nq in (0, 1, 4096, 10 ** 9):
        assert lib.rae_rank_workspace_bytes(C.byref(_rank_args(lib, nq=nq)), None) == base

    def strips(n):
        tiles = -(-n // _lib.RAE_RK_TE)
        per_strip = -(-tiles // _lib.RAE_RK_MAXSTRIPS)
        return -(-tiles // per_strip)
    for n in (1, 128, 129, 128 * 128, 128 * 128 + 1, 10 ** 6, (1 << 31) - 1):
        got = lib.rae_rank_workspace_bytes(C.byref(_rank_args(lib, n_entities=n)), None)
        assert got == strips(n) * _lib.RAE_RK_QCHUNK * 8, (n, got)
        assert strips(n) <= _lib.RAE_RK_MAXSTRIPS
    assert lib.rae_rank_workspace_bytes(C.byref(_rank_args(lib, n_entities=0)), None) == -1
    assert lib.rae_rank_workspace_bytes(C.byref(_rank_args(lib, embed=1025)), None) == -1
    for dec in ("sp", "rescal", "rescal+sp"):
        b0 = lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, dec)))
        assert b0 > 0
        for nrows in (0, 1, 2048, 2065, 10 ** 8):
            assert lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, dec, nrows=nrows))) == b0
        big = lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, dec, n_entities=(1 << 31) - 1)))
        cap = lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, dec, n_entities=128 * 128)))
        assert big == cap                                 # bounded by the strip count
    assert lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, "sp", n_entities=0))) == -1
    assert lib.rae_rank_workspace_bytes(None, C.byref(_eval_args(lib, "rescal", relations=324))) == -1
