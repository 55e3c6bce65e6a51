"""Host side of the top-k entity retrieval (rae_topk_queries, rae_eval_topk, include/rae.h): the
numpy oracle on hand cases, the ctypes struct layouts against the C compiler, the argument checks
(they run before any HIP call, so they work without a GPU), the bounded workspace, the formatters
and the command line flags.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from _rank_ref import DEC_ID

INF = np.inf


# ------------------------------------------------------------------------ 1. the oracle
def test_topk_from_scores_ties_are_broken_by_entity():
    from rae.evaluation import topk_from_scores
    g = np.array([[1.0, 3.0, 3.0, 0.5, 3.0],
                  [2.0, 2.0, 2.0, 2.0, 2.0]])
    e, s = topk_from_scores(g, 3)
    assert e.dtype == np.int32 and e.tolist() == [[1, 2, 4], [0, 1, 2]]
    assert s.tolist() == [[3.0, 3.0, 3.0], [2.0, 2.0, 2.0]]
    e, s = topk_from_scores(g, 4)
    assert e.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and s[0].tolist() == [3.0, 3.0, 3.0, 1.0]
    e, _ = topk_from_scores(g, 1)
    assert e.tolist() == [[1], [0]]


def test_topk_from_scores_pads_when_top_exceeds_n():
    from rae.evaluation import topk_from_scores
    e, s = topk_from_scores(np.array([[0.5, -1.0]]), 4)
    assert e.tolist() == [[0, 1, -1, -1]]
    assert s.tolist() == [[0.5, -1.0, -INF, -INF]]
    e, s = topk_from_scores(np.zeros((0, 3)), 2)
    assert e.shape == (0, 2) and s.shape == (0, 2)
    # a real -inf score is a candidate and sorts before the padding
    e, s = topk_from_scores(np.array([[-INF, 1.0]]), 3)
    assert e.tolist() == [[1, 0, -1]] and s.tolist() == [[1.0, -INF, -INF]]


def test_topk_from_scores_skip_in_and_out_of_range():
    from rae.evaluation import topk_from_scores
    g = np.array([[5.0, 4.0, 3.0]] * 6)
    skip = np.array([0, 2, -1, 3, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
    e, s = topk_from_scores(g, 3, skip)
    assert e.tolist() == [[1, 2, -1], [0, 1, -1], [0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert s[0].tolist() == [4.0, 3.0, -INF]
    assert topk_from_scores(g, 3, skip.astype(np.int32))[0].tolist() == e.tolist()


def test_topk_from_scores_leaves_nan_out_and_makes_negative_zero_positive():
    from rae.evaluation import topk_from_scores
    g = np.array([[np.nan, -0.0, 0.0, -1.0, np.nan, INF],
                  [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]])
    e, s = topk_from_scores(g, 4)
    assert e.tolist() == [[5, 1, 2, 3], [-1, -1, -1, -1]]     # -0 == +0: entity 1 before 2
    assert s[0].tolist() == [INF, 0.0, 0.0, -1.0] and not np.signbit(s[0, 1:3]).any()
    assert np.isneginf(s[1]).all()
    e32, s32 = topk_from_scores(g.astype(np.float32), 6)
    assert s32.dtype == np.float32 and e32[0].tolist() == [5, 1, 2, 3, -1, -1]


# ----------------------------------------------------------------- 2. the struct layouts
@pytest.mark.parametrize("cname,pyname", [("rae_topk_args", "RaeTopkArgs"),
                                          ("rae_topk_out", "RaeTopkOut")])
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
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.split("\n") if line)
    assert int(got["size"]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname


def test_constants_are_the_kernels():
    from rae import _lib
    hpp = open(os.path.join(_lib.CSRC, "rae_topk.hpp")).read()
    assert f"#define RAE_ETK_QCHUNK {_lib.RAE_ETK_QCHUNK} " in hpp
    assert f"#define RAE_ETK_MAXTOP {_lib.RAE_ETK_MAXTOP} " in hpp
    for sym in ("rae_topk_queries", "rae_eval_topk", "rae_topk_workspace_bytes"):
        assert sym in _lib.EXPORTS


# -------------------------------------------------------------- 3. rejection without a GPU
_KEEP = []
INVALID = -1                                                   # RAE_E_INVALID


def _buf(nbytes, align=256, offset=0):
    """A host address with the given alignment (never dereferenced: every case is rejected, or
    is a workspace-bytes query, before a HIP call)."""
    raw = C.create_string_buffer(nbytes + align + 16)
    _KEEP.append(raw)
    base = C.addressof(raw)
    return ((base + align - 1) // align) * align + offset


def _topk_args(lib, **kw):
    from rae import _lib
    a = _lib.RaeTopkArgs()
    a.Q, a.ldq, a.nq = _buf(4096), 16, 8
    a.add, a.skip = _buf(64), _buf(64)
    a.A, a.Ab, a.n_entities, a.embed = _buf(4096), _buf(64), 10, 16
    a.top = 5
    a.ents_out, a.scores_out = _buf(256), _buf(256)
    need = lib.rae_topk_workspace_bytes(C.byref(a), None, a.top)
    assert need > 0
    a.workspace, a.workspace_bytes = _buf(16), need
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _eval_args(lib, dec="sp", top=5, **kw):
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
    need = lib.rae_topk_workspace_bytes(None, C.byref(a), top)
    a.workspace, a.workspace_bytes = _buf(16), max(need, 0)
    return a


def _topk_out(top=5, **kw):
    from rae import _lib
    o = _lib.RaeTopkOut()
    o.ents, o.scores, o.top, o.skip_true = _buf(256), _buf(256), top, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


TOPK_BAD = [
    dict(top=0), dict(top=33), dict(top=-1),
    dict(ldq=18), dict(ldq=12),                                # ldq % 4, ldq < embed
    dict(embed=0), dict(embed=1025, ldq=1028),
    dict(n_entities=0), dict(n_entities=1 << 31),
    dict(Q=_buf(4096, 256, 4)), dict(workspace=_buf(4096, 256, 64)),
    dict(A=_buf(4096, 256, 8)),
    dict(workspace_bytes=0), dict(ents_out=None),
    dict(Q=None), dict(A=None), dict(workspace=None), dict(nq=-1),
]


@pytest.mark.parametrize("bad", TOPK_BAD, ids=lambda b: "-".join(f"{k}{v}" if isinstance(v, int)
                                                                  and abs(v) < 4096 else f"{k}"
                                                                  for k, v in b.items()))
def test_topk_queries_rejects(built_lib, bad):
    a = _topk_args(built_lib)
    if "workspace_bytes" in bad:
        bad = dict(workspace_bytes=a.workspace_bytes - 1)      # one byte too small
    for k, v in bad.items():
        setattr(a, k, v)
    assert built_lib.rae_topk_queries(C.byref(a), None) == INVALID, bad
    assert built_lib.rae_last_error()


def test_null_structs_are_rejected(built_lib):
    lib = built_lib
    assert lib.rae_topk_queries(None, None) == INVALID and lib.rae_last_error()
    assert lib.rae_eval_topk(None, C.byref(_topk_out()), None) == INVALID and lib.rae_last_error()
    assert lib.rae_eval_topk(C.byref(_eval_args(lib)), None, None) == INVALID
    assert lib.rae_last_error()
    assert lib.rae_eval_topk(None, None, None) == INVALID


def test_nq_zero_reads_no_pointer(built_lib):
    """nq == 0 returns before any pointer is looked at (and before any HIP call)."""
    a = _topk_args(built_lib, nq=0, Q=None, A=None, ents_out=None, workspace=None,
                   workspace_bytes=0)
    assert built_lib.rae_topk_queries(C.byref(a), None) == 0


EVAL_BAD = [
    ("sp", dict(decoder=3)), ("sp", dict(decoder=-1)),
    ("sp", dict(W=None)), ("sp", dict(A=None)), ("sp", dict(Ab=None)), ("sp", dict(C1=None)),
    ("rescal+sp", dict(C2=None)), ("rescal", dict(R3=None)),
    ("sp", dict(indptr=None)), ("sp", dict(args1=None)), ("sp", dict(workspace=None)),
    ("sp", dict(embed=0)), ("sp", dict(embed=1025)),
    ("sp", dict(n_entities=0)), ("sp", dict(n_entities=1 << 31)),
    ("sp", dict(nrows=-1)), ("sp", dict(row0=-1)), ("sp", dict(relations=0)),
    ("rescal", dict(relations=324)),
    ("sp", dict(A=_buf(64, 256, 4))), ("sp", dict(W=_buf(64, 256, 4))),
]


@pytest.mark.parametrize("dec,bad", EVAL_BAD, ids=lambda b: "-".join(b) if isinstance(b, dict) else b)
def test_eval_topk_rejects(built_lib, dec, bad):
    a = _eval_args(built_lib, dec)
    for k, v in bad.items():
        setattr(a, k, v)
    assert built_lib.rae_eval_topk(C.byref(a), C.byref(_topk_out()), None) == INVALID, (dec, bad)
    assert built_lib.rae_last_error()


def test_eval_topk_rejects_outputs_and_workspace(built_lib):
    lib = built_lib
    a = _eval_args(lib)
    for top in (0, 33):
        assert lib.rae_eval_topk(C.byref(a), C.byref(_topk_out(top=top)), None) == INVALID
        assert b"top" in lib.rae_last_error()
    assert lib.rae_eval_topk(C.byref(a), C.byref(_topk_out(ents=None)), None) == INVALID
    assert lib.rae_last_error()
    short = _eval_args(lib)
    short.workspace_bytes -= 1
    assert lib.rae_eval_topk(C.byref(short), C.byref(_topk_out()), None) == INVALID
    assert b"workspace_bytes" in lib.rae_last_error()
    small = _eval_args(lib, top=1)                        # sized for top = 1, asked for 5
    assert small.workspace_bytes > 0
    assert lib.rae_eval_topk(C.byref(small), C.byref(_topk_out(top=5)), None) == INVALID
    mis = _eval_args(lib)
    mis.workspace = _buf(4096, 256, 128)
    assert lib.rae_eval_topk(C.byref(mis), C.byref(_topk_out()), None) == INVALID
    assert b"256-byte" in lib.rae_last_error()
    # nrows == 0 is valid, writes nothing and needs no output pointer
    empty = _eval_args(lib, nrows=0)
    assert lib.rae_eval_topk(C.byref(empty), C.byref(_topk_out(ents=None, scores=None)), None) == 0


# ------------------------------------------------------------------- 4. workspace bytes
def test_workspace_bytes_without_a_gpu(built_lib):
    from rae import _lib
    lib = built_lib
    MiB = 1 << 20
    assert lib.rae_topk_workspace_bytes(None, None, 5) == -1
    a, e = _topk_args(lib), _eval_args(lib)
    assert lib.rae_topk_workspace_bytes(C.byref(a), C.byref(e), 5) == -1
    big = lib.rae_topk_workspace_bytes(C.byref(_topk_args(lib, n_entities=(1 << 31) - 1)), None, 32)
    assert 0 < big <= 32 * MiB
    # independent of nq and of the pointers
    base = lib.rae_topk_workspace_bytes(C.byref(a), None, 5)
    for nq in (0, 1, 1024, 1041, 10 ** 9):
        assert lib.rae_topk_workspace_bytes(C.byref(_topk_args(lib, nq=nq)), None, 5) == base

    def strips(n):
        tiles = -(-n // _lib.RAE_RK_TE)
        per_strip = -(-tiles // _lib.RAE_RK_MAXSTRIPS)
        return -(-tiles // per_strip)
    for n in (1, 128, 129, 128 * 128, 128 * 128 + 1, 10 ** 6, (1 << 31) - 1):
        for top in (1, 10, 32):
            got = lib.rae_topk_workspace_bytes(C.byref(_topk_args(lib, n_entities=n)), None, top)
            assert got == strips(n) * _lib.RAE_ETK_QCHUNK * top * 8, (n, top, got)
    for top in (0, 33):
        assert lib.rae_topk_workspace_bytes(C.byref(a), None, top) == -1
        assert lib.rae_topk_workspace_bytes(None, C.byref(e), top) == -1
    assert lib.rae_topk_workspace_bytes(C.byref(_topk_args(lib, n_entities=0)), None, 5) == -1
    assert lib.rae_topk_workspace_bytes(C.byref(_topk_args(lib, embed=1025)), None, 5) == -1
    for dec in ("sp", "rescal", "rescal+sp"):
        b0 = lib.rae_topk_workspace_bytes(None, C.byref(_eval_args(lib, dec)), 5)
        assert b0 > base
        for nrows in (0, 1, 2048, 2065, 10 ** 8):
            assert lib.rae_topk_workspace_bytes(None, C.byref(_eval_args(lib, dec, nrows=nrows)), 5) == b0
        far = lib.rae_topk_workspace_bytes(None, C.byref(_eval_args(lib, dec, n_entities=(1 << 31) - 1)), 5)
        cap = lib.rae_topk_workspace_bytes(None, C.byref(_eval_args(lib, dec, n_entities=128 * 128)), 5)
        assert far == cap                                 # bounded by the strip count
    assert lib.rae_topk_workspace_bytes(None, C.byref(_eval_args(lib, "rescal", relations=324)), 5) == -1


# ------------------------------------------------------------------------ 5. formatters
def test_formatters_on_a_hand_case():
    from rae.evaluation import format_argument_predictions, format_relation_preferences
    names = {0: "Ada Lovelace", 1: "The Notes", 3: "a:b"}
    ents = np.array([[[1, 0, -1]], [[2, 3, 0]]], dtype=np.int32)          # (2, m = 1, top = 3)
    scores = np.array([[[1.5, -0.25, -INF]], [[np.float32(0.1), 0.0, -2.0]]], dtype=np.float32)
    lines = format_relation_preferences(ents, scores, names)
    assert lines == ["preferences\t0\t1\tThe Notes:1.5\tAda Lovelace:-0.25",
                     "preferences\t0\t2\t2:0.100000001\ta:b:0\tAda Lovelace:-2"]
    # the printed score gives the float32 back
    name, val = lines[1].split("\t")[3].rsplit(":", 1)
    assert name == "2" and np.float32(float(val)) == np.float32(0.1)
    assert format_relation_preferences(ents, scores)[0] == "preferences\t0\t1\t1:1.5\t0:-0.25"
    pe = np.array([[[1, 0], [0, 1]], [[3, 1], [-1, -1]]], dtype=np.int32)  # (2 rows, 2, top 2)
    ps = np.array([[[2.0, 1.0], [0.5, 0.25]], [[3.0, -1.0], [-INF, -INF]]], dtype=np.float32)
    true = np.array([[0, 1], [3, 2]])
    lines = format_argument_predictions(pe, ps, true, names, row0=7)
    assert lines == ["predictions\t7\t1\tAda Lovelace\tThe Notes:2\tAda Lovelace:1",
                     "predictions\t7\t2\tThe Notes\tAda Lovelace:0.5\tThe Notes:0.25",
                     "predictions\t8\t1\ta:b\ta:b:3\tThe Notes:-1",
                     "predictions\t8\t2\t2"]


# --------------------------------------------------------------------------- 6. the flags
def test_cli_flags_parse_and_default_off():
    from rae.cli import get_command_args
    base = ["data.npz", "--model-name", "m", "--decoder", "sp"]
    a = get_command_args(base)
    assert a.print_preferences == 0 and a.predict_arguments == 0 and a.predict_top == 10
    a = get_command_args(base + ["--print-preferences"])
    assert a.print_preferences == 5
    a = get_command_args(base + ["--print-preferences", "3", "--predict-arguments", "20",
                                 "--predict-top", "7"])
    assert (a.print_preferences, a.predict_arguments, a.predict_top) == (3, 20, 7)
    with pytest.raises(SystemExit):
        get_command_args(base + ["--predict-arguments"])


def test_inducer_refuses_bad_values_before_touching_a_device():
    from rae import inducer
    mk = lambda dec, **kw: inducer.ReconstructInducer(
        None, {}, None, 1, 0.1, 10, 4, 3, 2, 0.0, 0.0, "adagrad", "m", dec, False, True, False,
        1.0, **kw)
    with pytest.raises(ValueError, match="print_preferences"):
        mk("sp", print_preferences=33)
    with pytest.raises(ValueError, match="print_preferences"):
        mk("rescal", print_preferences=3)
    with pytest.raises(ValueError, match="predict_top"):
        mk("sp", predict_arguments=4, predict_top=0)
