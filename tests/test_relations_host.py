"""Host side of the decoder's relation scores (rae_relation_scores, rae_eval_relations,
include/rae.h): the definition pinned to what already exists (the objective's positive score),
hand cases, the ctypes struct layouts against the C compiler, the argument checks (they run before
any HIP call, so they work without a GPU), the workspace query, the inputs of the GPU tests
(float32 restatement within half of their bounds; integer partial sums below 2^24), the formatter
and the command line flags.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import rae_oracle as O
from conftest import ROOT
from _entry_ref import group
from _rank_ref import queries64
from _rel_ref import (DEC_ID, DECODERS, EVAL_CASES, FLOAT_SHAPES, ell64, eval_problem,
                      float_params, int_pairs, int_params, joint32, joint64, joint_bound,
                      logsoftmax64, max_partial_magnitude, psi32, psi64, psi_bound)

INVALID = -1                                                   # RAE_E_INVALID


# ------------------------------------------------------ 1. the definition is what already exists
def _problem(dec, seed=0, l=12, d=20, m=5, n=9, r=4):
    g = np.random.RandomState(seed)
    f = lambda *shape: g.standard_normal(shape) * 0.7
    p = {"W": f(d, m), "Wb": f(m), "A": f(n, r), "Ab": f(n)}
    if dec != "rescal":
        p["C1"], p["C2"] = f(r, m), f(r, m)
    if dec != "sp":
        p["R" if dec == "rescal" else "C"] = f(r, r, m)
    X = sp.csr_matrix((g.rand(l, d) < 0.3).astype(np.float64))
    e1, e2 = g.randint(0, n, l), g.randint(0, n, l)
    return p, X, e1, e2


@pytest.mark.parametrize("dec", DECODERS)
def test_expected_psi_is_the_positive_score(dec):
    p, X, e1, e2 = _problem(dec)
    S = np.asarray(X @ p["W"]) + p["Wb"]
    P = np.exp(logsoftmax64(S))
    psi = psi64(dec, p, e1, e2)
    _, _, u, _ = queries64(dec, p, X, e1, e2)
    one = u[:, 0] - p["Ab"][e1]
    np.testing.assert_allclose((P * psi).sum(axis=1), one, rtol=1e-12, atol=1e-13)
    # rae.evaluation's oracle is the same function
    from rae.evaluation import relation_scores
    np.testing.assert_allclose(relation_scores(p, dec, e1, e2), psi, rtol=1e-13, atol=1e-14)
    other = (e2 + 1) % p["A"].shape[0]
    if dec == "sp":                  # A[args1] twice: psi does not see e2
        assert np.array_equal(psi64(dec, p, e1, other), psi)
    else:
        assert not np.allclose(psi64(dec, p, e1, other), psi)
    if dec == "rescal+sp":           # the hybrid's C2 term is a2's
        a1, a2 = p["A"][e1], p["A"][e2]
        want = np.einsum("bi,ijk,bj->bk", a1, p["C"], a2) + a1 @ p["C1"] + a2 @ p["C2"]
        np.testing.assert_allclose(psi, want, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("dec", DECODERS)
def test_ell_at_a_one_hot_relation_is_the_oracles_pos_term(dec):
    p, X, e1, e2 = _problem(dec, seed=1)
    l, m = len(e1), p["Wb"].shape[0]
    psi = psi64(dec, p, e1, e2)
    ell = ell64(psi, p["Ab"], e1, e2)
    neg = np.zeros((1, l), np.int64)
    for k in range(m):
        q = dict(p, W=np.zeros_like(p["W"]), Wb=np.where(np.arange(m) == k, 800.0, 0.0))
        res = O.train_step_grads(dec, q, X, e1, e2, neg, neg, alpha=1.0)
        pos = group(dec, res.scores, l, 1)[:, 0]
        np.testing.assert_allclose(ell[:, k], pos, rtol=1e-12, atol=1e-13)


def test_joint_scores_oracle():
    from rae.evaluation import joint_scores
    p, X, e1, e2 = _problem("rescal+sp", seed=2)
    psi, lsm, ell, J = joint64("rescal+sp", p, X, e1, e2)
    S = np.asarray(X @ p["W"]) + p["Wb"]
    np.testing.assert_allclose(joint_scores(S, psi, p["Ab"], e1, e2), J, rtol=1e-13, atol=1e-14)
    sat = joint_scores(np.array([[0.0, 2000.0]]), np.zeros((1, 2)), np.zeros(3), [0], [1])
    assert np.isfinite(sat).all() and sat[0, 0] == pytest.approx(-2000.0 + 2 * np.log(0.5))


# ------------------------------------------------------------------------- 2. hand cases
A_H = np.array([[1.0, 2.0], [3.0, -1.0], [0.0, 0.5]])
C1_H = np.array([[1.0, 0.0, -1.0], [2.0, 1.0, 0.0]])           # (r, m)
C2_H = np.array([[0.0, 1.0, 1.0], [-1.0, 0.0, 2.0]])
R_H = np.zeros((2, 2, 3))
R_H[:, :, 0] = [[1, 0], [0, 1]]                                # a1 . a2
R_H[:, :, 1] = [[0, 1], [0, 0]]                                # a1[0] a2[1]
R_H[:, :, 2] = [[2, 0], [1, -1]]                               # 2 a1[0]a2[0] + a1[1]a2[0] - a1[1]a2[1]


def test_hand_cases():
    e1, e2 = np.array([0, 1]), np.array([1, 2])
    # pair 0: a1 = (1, 2), a2 = (3, -1);  pair 1: a1 = (3, -1), a2 = (0, 0.5)
    sp_ = psi64("sp", {"A": A_H, "C1": C1_H, "C2": C2_H}, e1, e2)
    #   <C1[:,k], a1> = (1+4, 0+2, -1+0) = (5, 2, -1);  <C2[:,k], a1> = (0-2, 1+0, 1+4) = (-2, 1, 5)
    #   pair 1: (3-2, 0-1, -3+0) = (1, -1, -3);           (0+1, 3+0, 3-2) = (1, 3, 1)
    assert sp_.tolist() == [[3.0, 3.0, 4.0], [2.0, 2.0, -2.0]]
    res = psi64("rescal", {"A": A_H, "R": R_H}, e1, e2)
    #   pair 0: (3-2, 1*-1, 2*3 + 2*3 - 2*-1) = (1, -1, 14)
    #   pair 1: (0 - 0.5, 3*0.5, 0 + 0 - (-1*0.5)) = (-0.5, 1.5, 0.5)
    assert res.tolist() == [[1.0, -1.0, 14.0], [-0.5, 1.5, 0.5]]
    hyb = psi64("rescal+sp", {"A": A_H, "C": R_H, "C1": C1_H, "C2": C2_H}, e1, e2)
    #   + <C1[:,k], a1> as above, + <C2[:,k], a2>: pair 0 a2 = (3,-1): (0+1, 3+0, 3-2) = (1, 3, 1)
    #   pair 1 a2 = (0, 0.5): (-0.5, 0, 1)
    assert hyb.tolist() == [[1.0 + 5 + 1, -1.0 + 2 + 3, 14.0 - 1 + 1],
                            [-0.5 + 1 - 0.5, 1.5 - 1 + 0, 0.5 - 3 + 1]]
    from rae.evaluation import relation_scores
    assert relation_scores({"A": A_H, "R": R_H}, "rescal", e1, e2).tolist() == res.tolist()
    with pytest.raises(IndexError):
        relation_scores({"A": A_H, "R": R_H}, "rescal", [3], [0])
    with pytest.raises(IndexError):
        relation_scores({"A": A_H, "R": R_H}, "rescal", [0], [-1])


# ----------------------------------------------------------------- 3. the struct layouts
@pytest.mark.parametrize("cname,pyname", [("rae_relscore_args", "RaeRelscoreArgs"),
                                          ("rae_rel_out", "RaeRelOut")])
def test_struct_layout_matches_c_compiler(tmp_path, cname, pyname):
    from rae import _lib
    st = getattr(_lib, pyname)
    src = tmp_path / "off.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rae.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "off"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.split("\n") if line)
    assert int(got["size"]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname


def test_exports_and_constants():
    from rae import _lib
    for sym in ("rae_relation_scores", "rae_eval_relations", "rae_relscore_workspace_bytes"):
        assert sym in _lib.EXPORTS
    hpp = open(os.path.join(_lib.CSRC, "rae_relscore.hpp")).read()
    assert f"#define RAE_RS_ROUND {_lib.RAE_RS_ROUND} " in hpp
    assert f"#define RAE_RS_TK {_lib.RAE_RS_TK} " in hpp


# -------------------------------------------------------------- 4. rejection without a GPU
_KEEP = []


def _buf(nbytes, align=256, offset=0):
    """A host address with the given alignment (never dereferenced: every case is rejected, or
    is a workspace-bytes query, before a HIP call)."""
    raw = C.create_string_buffer(nbytes + align + 16)
    _KEEP.append(raw)
    base = C.addressof(raw)
    return ((base + align - 1) // align) * align + offset


def _rel_args(dec="rescal+sp", **kw):
    from rae import _lib
    a = _lib.RaeRelscoreArgs()
    a.decoder, a.relations, a.embed, a.n_entities = DEC_ID[dec], 8, 16, 10
    a.A, a.C1, a.C2, a.R3 = _buf(64), _buf(64), _buf(64), _buf(64)
    a.e1, a.e2, a.nq = _buf(64), _buf(64), 4
    a.psi_out, a.ldp = _buf(256), 8
    a.workspace, a.workspace_bytes = None, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _eval_args(lib, dec="rescal+sp", **kw):
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
    need = lib.rae_relscore_workspace_bytes(None, C.byref(a))
    a.workspace, a.workspace_bytes = _buf(16), max(need, 0)
    return a


def _rel_out(**kw):
    from rae import _lib
    o = _lib.RaeRelOut()
    o.psi, o.joint, o.labels_dec, o.labels_joint = _buf(256), _buf(256), _buf(64), _buf(64)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


REL_BAD = [
    ("rescal+sp", dict(decoder=3)), ("sp", dict(decoder=-1)),
    ("rescal+sp", dict(A=None)), ("sp", dict(C1=None)), ("rescal+sp", dict(C2=None)),
    ("rescal", dict(R3=None)), ("rescal+sp", dict(R3=None)),
    ("sp", dict(e1=None)), ("sp", dict(e2=None)), ("sp", dict(psi_out=None)),
    ("sp", dict(ldp=7)), ("sp", dict(nq=-1)),
    ("sp", dict(relations=0)), ("sp", dict(relations=513)), ("sp", dict(relations=130, ldp=130)),
    ("rescal", dict(relations=324, ldp=324)), ("rescal+sp", dict(relations=512, ldp=512)),
    ("sp", dict(embed=0)), ("sp", dict(embed=1025)),
    ("sp", dict(n_entities=0)), ("sp", dict(n_entities=1 << 31)),
    ("rescal", dict(R3=_buf(64, 256, 4))), ("sp", dict(C1=_buf(64, 256, 8))),
    ("sp", dict(workspace=_buf(64, 256, 64))), ("sp", dict(workspace_bytes=-1)),
]


@pytest.mark.parametrize("dec,bad", REL_BAD,
                         ids=lambda b: "-".join(b) if isinstance(b, dict) else b)
def test_relation_scores_rejects(built_lib, dec, bad):
    a = _rel_args(dec, **bad)
    assert built_lib.rae_relation_scores(C.byref(a), None) == INVALID, (dec, bad)
    assert built_lib.rae_last_error()
    assert built_lib.rae_relation_scores(None, None) == INVALID


def test_nq_zero_reads_no_pointer(built_lib):
    a = _rel_args(nq=0, A=None, C1=None, C2=None, R3=None, e1=None, e2=None, psi_out=None)
    assert built_lib.rae_relation_scores(C.byref(a), None) == 0
    e = _eval_args(built_lib, nrows=0, row0=7)
    assert built_lib.rae_eval_relations(C.byref(e), C.byref(_rel_out()), None) == 0


EVAL_BAD = [
    ("sp", dict(decoder=3)), ("sp", dict(W=None)), ("sp", dict(Wb=None)), ("sp", dict(A=None)),
    ("sp", dict(Ab=None)), ("sp", dict(C1=None)), ("rescal+sp", dict(C2=None)),
    ("rescal", dict(R3=None)), ("sp", dict(indptr=None)), ("sp", dict(indices=None)),
    ("sp", dict(args1=None)), ("sp", dict(args2=None)), ("sp", dict(workspace=None)),
    ("sp", dict(workspace=_buf(1 << 12, 256, 64))),
    ("sp", dict(embed=0)), ("sp", dict(embed=1025)), ("sp", dict(relations=0)),
    ("sp", dict(relations=516)), ("rescal", dict(relations=324)),
    ("sp", dict(n_entities=0)), ("sp", dict(n_entities=1 << 31)),
    ("sp", dict(nrows=-1)), ("sp", dict(row0=-1)), ("sp", dict(row0=(1 << 31) - 2)),
    ("sp", dict(A=_buf(64, 256, 4))), ("sp", dict(W=_buf(64, 256, 4))),
]


@pytest.mark.parametrize("dec,bad", EVAL_BAD,
                         ids=lambda b: "-".join(b) if isinstance(b, dict) else b)
def test_eval_relations_rejects(built_lib, dec, bad):
    a = _eval_args(built_lib, dec)
    for k, v in bad.items():
        setattr(a, k, v)
    assert built_lib.rae_eval_relations(C.byref(a), C.byref(_rel_out()), None) == INVALID, bad
    assert built_lib.rae_last_error()


def test_eval_relations_rejects_outputs_and_workspace(built_lib):
    lib = built_lib
    a = _eval_args(lib)
    none = _rel_out(psi=None, joint=None, labels_dec=None, labels_joint=None)
    assert lib.rae_eval_relations(C.byref(a), C.byref(none), None) == INVALID
    assert b"outputs" in lib.rae_last_error()
    assert lib.rae_eval_relations(C.byref(a), None, None) == INVALID and lib.rae_last_error()
    assert lib.rae_eval_relations(None, C.byref(_rel_out()), None) == INVALID
    short = _eval_args(lib)
    short.workspace_bytes -= 1
    assert lib.rae_eval_relations(C.byref(short), C.byref(_rel_out()), None) == INVALID
    assert b"workspace_bytes" in lib.rae_last_error()


def test_workspace_bytes(built_lib):
    lib = built_lib
    q, e = _rel_args(), _eval_args(lib)
    assert lib.rae_relscore_workspace_bytes(None, None) == -1 and lib.rae_last_error()
    assert lib.rae_relscore_workspace_bytes(C.byref(q), C.byref(e)) == -1
    assert lib.rae_relscore_workspace_bytes(C.byref(q), None) == 0
    need = lib.rae_relscore_workspace_bytes(None, C.byref(e))
    assert need >= 2 * 16384 * 8 * 4
    for nq in (0, 1, 1 << 20, 1 << 40):
        q.nq = nq
        assert lib.rae_relscore_workspace_bytes(C.byref(q), None) == 0
    for nrows in (0, 1, 1 << 20, (1 << 31) - 1):
        e.nrows = nrows
        assert lib.rae_relscore_workspace_bytes(None, C.byref(e)) == need
    assert lib.rae_relscore_workspace_bytes(C.byref(_rel_args(embed=1025)), None) == -1
    assert lib.rae_relscore_workspace_bytes(C.byref(_rel_args("rescal", relations=324)), None) == -1
    assert lib.rae_relscore_workspace_bytes(None, C.byref(_eval_args(lib, relations=516))) == -1


# ------------------------------------------------------------ 5. the inputs of the GPU tests
@pytest.mark.parametrize("r,m", FLOAT_SHAPES)
@pytest.mark.parametrize("dec", DECODERS)
def test_float_inputs_leave_half_the_bound(dec, r, m):
    """tests/test_gpu_relations.py test_float_psi_within_the_derived_bound's inputs: a float32
    numpy evaluation stays within half of the bound the kernel is held to."""
    n, nq = 40, 150
    p = float_params(11, dec, n, r, m)
    e1, e2 = int_pairs(5, n, nq)
    err = np.abs(psi32(dec, p, e1, e2).astype(np.float64) - psi64(dec, p, e1, e2))
    bound = psi_bound(dec, p, e1, e2)
    print(f"{dec} r {r} m {m}: float32 restatement max err / bound {(err / bound).max():.3e}")
    assert (err <= bound / 2).all()


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: f"{c[0]}-m{c[1]}-r{c[2]}")
def test_joint_inputs_leave_half_the_bound(case):
    dec, m, r, rows = case
    prob = eval_problem(dec, m, r, rows)
    psi, J = joint32(dec, prob.p32, prob.X, prob.a1, prob.a2)
    _, _, _, J64 = joint64(dec, prob.p64, prob.X, prob.a1, prob.a2)
    epsi = np.abs(psi.astype(np.float64) - psi64(dec, prob.p64, prob.a1, prob.a2))
    assert (epsi <= psi_bound(dec, prob.p64, prob.a1, prob.a2) / 2).all()
    err = np.abs(J.astype(np.float64) - J64)
    bound = joint_bound(dec, prob.p64, prob.X, prob.a1, prob.a2)
    print(f"{dec} m {m} r {r}: float32 restatement max |dJ| / bound {(err / bound).max():.3e}")
    assert (err <= bound / 2).all()


@pytest.mark.parametrize("dec", DECODERS)
def test_integer_cases_stay_below_2_24(dec):
    """Every partial sum of the exact cases is an integer below 2^24 in magnitude, so fp32 holds
    it exactly whatever the order of summation: the largest shapes of each kind."""
    for r, m, n in ((257, 320, 9), (257, 100, 9), (200, 100, 9), (1024, 4, 5), (33, 512, 9)):
        if dec != "sp" and m > 320:
            continue
        p = int_params(7 * r + m, dec, n, r, m)
        assert all(np.array_equal(v, np.round(v)) for v in p.values())
        assert max_partial_magnitude(dec, p) < 2 ** 24, (dec, r, m)


# ------------------------------------------------------------------ 6. formatter and CLI
def test_format_relation_predictions():
    from rae.evaluation import format_relation_predictions
    psi = np.array([[0.5, 2.0, 2.0, -1.0], [1.0, 0.0, 0.25, 3.0]], dtype=np.float32)
    lines = format_relation_predictions([4, 0], [1, 4], [2, 0], [0.75, 0.5], psi, [1, 3], 3,
                                        names={0: "Paris", 1: "France", 4: "Seine"}, row0=10)
    assert lines == ["relations\t10\tSeine\tFrance\t2:0.75\t1:2\t2:2\t0:0.5\tjoint\t1",
                     "relations\t11\tParis\tSeine\t0:0.5\t3:3\t0:1\t2:0.25\tjoint\t3"]
    assert format_relation_predictions([], [], [], [], np.zeros((0, 4)), [], 2) == []
    # without names the ids are printed
    assert format_relation_predictions([7], [8], [0], [1.0], psi[:1], [2], 1)[0] == \
        "relations\t0\t7\t8\t0:1\t1:2\tjoint\t2"


def test_cli_flags_parse():
    from rae.cli import get_command_args
    base = ["ds.npz", "--model-name", "m", "--decoder", "sp"]
    a = get_command_args(base)
    assert a.label_with == "encoder" and a.predict_relations == 0
    for mode in ("encoder", "decoder", "joint"):
        assert get_command_args(base + ["--label-with", mode]).label_with == mode
    a = get_command_args(base + ["--predict-relations", "7", "--predict-top", "3"])
    assert a.predict_relations == 7 and a.predict_top == 3
    with pytest.raises(SystemExit):
        get_command_args(base + ["--label-with", "both"])
    with pytest.raises(SystemExit):
        get_command_args(base + ["--predict-relations", "x"])
