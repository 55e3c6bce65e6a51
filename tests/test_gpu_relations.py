"""rae_relation_scores / rae_eval_relations on the GPU (include/rae.h): exact psi on small-integer
data at the kernel's shape seams, float data against float64 within the derived bound of
tests/_rel_ref.py, the bitwise invariances the header states, the derived outputs (J, the two
labels), the tie to the objective's positive score on the device, and the engine / CLI surface on
the sample of tests/golden."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from _entry_ref import DeviceEval
from _rank_ref import DeviceRank
from _rel_ref import (DECODERS, EVAL_CASES, FLOAT_SHAPES, ROUND, DeviceRel, DeviceRelEval,
                      block_examples, eval_problem, float_params, int_pairs, int_params,
                      joint64, joint_bound, np_argmax_first, psi64, psi_bound)
from test_gpu_eval import TERM_ATOL, TERM_RTOL, _inducer, _params

pytestmark = pytest.mark.gpu

bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
same = lambda a, b: np.array_equal(bits(a), bits(b))


def test_constants_are_the_kernels():
    from rae import _lib
    src = open(os.path.join(PKG, "csrc", "rae_relscore.hpp")).read()
    assert f"#define RAE_RS_ROUND {_lib.RAE_RS_ROUND}" in src and _lib.RAE_RS_ROUND == ROUND
    assert f"#define RAE_RS_TK {_lib.RAE_RS_TK}" in src
    for m in (1, 16, 17, 100, 320, 512):
        assert _lib.relscore_block_examples(m) == block_examples(m)


# ------------------------------------------------------------------- 1. exact psi, integer data
R_GRID = (1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 200, 257)
M_GRID = (1, 3, 16, 17, 100)


def _exact(lib, dev, dec, r, m, nq, n=9, seed=0):
    p = int_params(seed + 7 * r + m, dec, n, r, m)
    e1, e2 = int_pairs(seed + r + m, n, nq)
    got = DeviceRel(lib, dev, dec, p).run(e1, e2)
    want = psi64(dec, p, e1, e2)
    assert got.shape == want.shape
    assert np.array_equal(got.astype(np.float64), want), (dec, r, m, nq,
                                                          np.abs(got - want).max())


@pytest.mark.parametrize("r", R_GRID)
@pytest.mark.parametrize("dec", DECODERS)
def test_exact_psi_over_the_shape_grid(built_lib, cuda_dev, dec, r):
    for m in M_GRID:
        _exact(built_lib, cuda_dev, dec, r, m, 130)      # > one example block of 64 and of 128


@pytest.mark.parametrize("dec", DECODERS)
def test_exact_psi_at_the_column_limit(built_lib, cuda_dev, dec):
    _exact(built_lib, cuda_dev, dec, 257, 320, 70)


def test_exact_psi_sp_beyond_one_column_group(built_lib, cuda_dev):
    _exact(built_lib, cuda_dev, "sp", 33, 512, 70)
    _exact(built_lib, cuda_dev, "sp", 33, 324, 70)


@pytest.mark.parametrize("dec", DECODERS)
def test_exact_psi_at_the_embed_limit(built_lib, cuda_dev, dec):
    _exact(built_lib, cuda_dev, dec, 1024, 4, 20, n=5)


@pytest.mark.parametrize("dec", DECODERS)
def test_exact_psi_over_the_pair_counts(built_lib, cuda_dev, dec):
    for r, m in ((3, 3), (5, 17)):
        be = block_examples(m)
        for nq in (0, 1, 15, 16, 17, be - 1, be, be + 1, ROUND - 1, ROUND, ROUND + 1):
            _exact(built_lib, cuda_dev, dec, r, m, nq)


# ------------------------------------------------------------------- 2. float data against float64
@pytest.mark.parametrize("r,m", FLOAT_SHAPES)
@pytest.mark.parametrize("dec", DECODERS)
def test_float_psi_within_the_derived_bound(built_lib, cuda_dev, dec, r, m):
    n, nq = 40, 150
    p = float_params(11, dec, n, r, m)
    e1, e2 = int_pairs(5, n, nq)
    got = DeviceRel(built_lib, cuda_dev, dec, p).run(e1, e2).astype(np.float64)
    want, bound = psi64(dec, p, e1, e2), psi_bound(dec, p, e1, e2)
    err = np.abs(got - want)
    print(f"{dec} r {r} m {m}: max |dpsi| {err.max():.3e}, max err / bound "
          f"{(err / bound).max():.3e} (|psi| max {np.abs(want).max():.3e})")
    assert (err <= bound).all()


# ------------------------------------------------------------------- 3. invariances, bitwise
@pytest.mark.parametrize("dec", DECODERS)
def test_rows_do_not_depend_on_count_position_or_neighbours(built_lib, cuda_dev, dec):
    n, nq, r, m = 40, 200, 33, 17
    p = float_params(2, dec, n, r, m)
    e1, e2 = int_pairs(9, n, nq)
    dr = DeviceRel(built_lib, cuda_dev, dec, p)
    base = dr.run(e1, e2)
    assert same(base, dr.run(e1, e2))                                 # the call repeated
    perm = np.random.RandomState(0).permutation(nq)
    assert same(base[perm], dr.run(e1[perm], e2[perm]))               # permuted
    assert same(base[37:129], dr.run(e1[37:129], e2[37:129]))         # a sub-range
    be = block_examples(m)
    rep = dr.run(np.full(be, e1[3]), np.full(be, e2[3]))              # every slot of a block
    assert same(rep, np.repeat(base[3:4], be, axis=0))
    # ldp > relations: the padding columns keep the sentinel
    wide = dr.run(e1, e2, ldp=m + 5, sentinel=-77.0)
    assert same(wide[:, :m], base) and (wide[:, m:] == -77.0).all()


@pytest.mark.parametrize("dec", DECODERS)
def test_ids_out_of_range_give_nan_rows_only(built_lib, cuda_dev, dec):
    n, nq, r, m = 40, 150, 33, 17
    p = float_params(4, dec, n, r, m)
    e1, e2 = int_pairs(1, n, nq)
    dr = DeviceRel(built_lib, cuda_dev, dec, p)
    base = dr.run(e1, e2)
    b1, b2 = e1.copy(), e2.copy()
    bad = {5: (-1, None), 64: (None, n), 65: (2 ** 31 - 1, None), 149: (None, -1), 70: (n, n)}
    for row, (x, y) in bad.items():
        if x is not None:
            b1[row] = x
        if y is not None:
            b2[row] = y
    got = dr.run(b1, b2)
    rows = sorted(bad)
    assert np.isnan(got[rows]).all()
    keep = np.setdiff1d(np.arange(nq), rows)
    assert same(got[keep], base[keep])


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: f"{c[0]}-m{c[1]}-r{c[2]}")
def test_eval_relations_is_relation_scores_on_any_row_range(built_lib, cuda_dev, case):
    dec, m, r, rows = case
    prob = eval_problem(dec, m, r, rows)
    de = DeviceEval(built_lib, prob, cuda_dev)
    dre = DeviceRelEval(de)
    dr = DeviceRel(built_lib, cuda_dev, dec, prob.p32)
    base = dr.run(prob.a1, prob.a2)
    full = dre.run(0, rows)
    assert same(full["psi"], base)
    for row0, nrows in ((0, 1), (7, 64), (63, 66), (rows - 1, 1), (rows, 0)):
        part = dre.run(row0, nrows)
        assert same(part["psi"], base[row0:row0 + nrows])
        assert same(part["joint"], full["joint"][row0:row0 + nrows])
        assert np.array_equal(part["labels_dec"], full["labels_dec"][row0:row0 + nrows])
        assert np.array_equal(part["labels_joint"], full["labels_joint"][row0:row0 + nrows])
    # psi in the workspace: the labels are the same
    only = dre.run(3, 100, want=("labels_dec", "labels_joint"))
    assert np.array_equal(only["labels_dec"], full["labels_dec"][3:103])
    assert np.array_equal(only["labels_joint"], full["labels_joint"][3:103])


def test_eval_relations_across_the_round_seam(built_lib, cuda_dev):
    """Rows on both sides of the launch round (16384) against rae_relation_scores."""
    from _entry_ref import EvalProblem
    g = np.random.RandomState(8)
    N = ROUND + 70
    prob = EvalProblem("rescal+sp", 8, 6, 1, list(g.randint(0, 4, size=N)), n=30, d=50, seed=4)
    de = DeviceEval(built_lib, prob, cuda_dev)
    dre = DeviceRelEval(de)
    base = DeviceRel(built_lib, cuda_dev, prob.dec, prob.p32).run(prob.a1, prob.a2)
    full = dre.run(0, N)
    assert same(full["psi"], base)
    part = dre.run(ROUND - 40, 110)
    for k in ("psi", "joint"):
        assert same(part[k], full[k][ROUND - 40:ROUND + 70])
    for k in ("labels_dec", "labels_joint"):
        assert np.array_equal(part[k], full[k][ROUND - 40:ROUND + 70])
    assert np.array_equal(full["labels_joint"], np_argmax_first(full["joint"]))


# ------------------------------------------------------------------- 4. derived outputs
@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: f"{c[0]}-m{c[1]}-r{c[2]}")
def test_joint_and_labels(built_lib, cuda_dev, case):
    dec, m, r, rows = case
    prob = eval_problem(dec, m, r, rows)
    out = DeviceRelEval(DeviceEval(built_lib, prob, cuda_dev)).run(0, rows)
    assert np.array_equal(out["labels_dec"], np_argmax_first(out["psi"]))
    assert np.array_equal(out["labels_joint"], np_argmax_first(out["joint"]))
    _, _, _, J = joint64(dec, prob.p64, prob.X, prob.a1, prob.a2)
    bound = joint_bound(dec, prob.p64, prob.X, prob.a1, prob.a2)
    err = np.abs(out["joint"].astype(np.float64) - J)
    print(f"{dec} m {m} r {r}: max |dJ| {err.max():.3e}, max err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


def test_labels_with_nan_and_ties(built_lib, cuda_dev):
    """numpy's argmax on the device: a NaN column wins over every number, the first NaN of an
    all-NaN row, the first of equal maxima."""
    dec, m, r, rows = "sp", 17, 8, 70
    prob = eval_problem(dec, m, r, rows)
    p = prob.p32
    p["A"][3, :] = np.nan                      # rows with entity 3 as e1: all-NaN psi
    p["A"][5, :] = 0.0                         # rows with entity 5 as e1: psi = 0 in every column
    p["W"][:] = 0.0                            # logits = Wb: with Wb constant, J ties too
    p["Wb"][:] = 0.25
    prob.a1[:8] = [3, 5, 3, 5, 1, 2, 5, 3]
    out = DeviceRelEval(DeviceEval(built_lib, prob, cuda_dev)).run(0, rows)
    assert np.isnan(out["psi"][0]).all() and (out["psi"][1] == 0).all()
    assert out["labels_dec"][0] == 0 and out["labels_joint"][0] == 0
    assert out["labels_dec"][1] == 0 and out["labels_joint"][1] == 0
    assert len(set(out["joint"][1].tolist())) == 1
    assert np.array_equal(out["labels_dec"], np_argmax_first(out["psi"]))
    assert np.array_equal(out["labels_joint"], np_argmax_first(out["joint"]))
    # one NaN column: it is the label of every row
    prob2 = eval_problem(dec, m, r, rows)
    prob2.p32["C1"][0, 11] = np.nan
    out2 = DeviceRelEval(DeviceEval(built_lib, prob2, cuda_dev)).run(0, rows)
    assert np.isnan(out2["psi"][:, 11]).all() and not np.isnan(np.delete(out2["psi"], 11, 1)).any()
    assert (out2["labels_dec"] == 11).all() and (out2["labels_joint"] == 11).all()


def test_saturated_row_has_a_finite_joint(built_lib, cuda_dev):
    """A logit gap above 104: fp32 P underflows to 0, log P would be -inf; J stays finite."""
    dec, m, r, rows = "rescal", 17, 8, 20
    prob = eval_problem(dec, m, r, rows)
    prob.p32["W"][:] = 0.0
    prob.p32["Wb"][:] = np.linspace(-150.0, 150.0, m).astype(np.float32)
    prob.p64 = {k: v.astype(np.float64) for k, v in prob.p32.items()}
    out = DeviceRelEval(DeviceEval(built_lib, prob, cuda_dev)).run(0, rows)
    assert np.isfinite(out["joint"]).all()
    _, lsm, _, J = joint64(dec, prob.p64, prob.X, prob.a1, prob.a2)
    assert lsm.min() < -104 and np.exp(lsm.min()).astype(np.float32) == 0
    bound = joint_bound(dec, prob.p64, prob.X, prob.a1, prob.a2)
    assert (np.abs(out["joint"].astype(np.float64) - J) <= bound).all()


# ------------------------------------------------------------------- 5. the tie to the objective
@pytest.mark.parametrize("dec", DECODERS)
def test_expected_psi_is_the_rank_target(built_lib, cuda_dev, dec):
    """sum_k P_k psi_k + Ab[args_t], in float64 from the device's psi and rae_label's probs,
    against rae_eval_rank's target."""
    import torch
    from rae import _lib
    m, r, rows = 17, 33, 150
    prob = eval_problem(dec, m, r, rows)
    de = DeviceEval(built_lib, prob, cuda_dev)
    psi = DeviceRelEval(de).run(0, rows, want=("psi",))["psi"].astype(np.float64)
    lab = torch.empty(rows, dtype=torch.int64, device=cuda_dev)
    pr = torch.empty((rows, m), dtype=torch.float32, device=cuda_dev)
    t = de.t
    _lib.check(built_lib.rae_label(
        C.c_void_p(t["indptr"].data_ptr()), C.c_void_p(t["indices"].data_ptr()),
        C.c_void_p(t["values"].data_ptr()), C.c_void_p(t["W"].data_ptr()),
        C.c_void_p(t["Wb"].data_ptr()), m, 0, rows, C.c_void_p(lab.data_ptr()),
        C.c_void_p(pr.data_ptr()), None), "rae_label")
    torch.cuda.synchronize()
    P = pr.cpu().numpy().astype(np.float64)
    one = (P * psi).sum(axis=1)
    Ab = prob.p64["Ab"]
    u = np.stack([one + Ab[prob.a1], one + Ab[prob.a2]], axis=1)
    _, _, tg, _, _ = DeviceRank(de).run(0, rows, summary=False)
    slack = (P * psi_bound(dec, prob.p64, prob.a1, prob.a2)).sum(axis=1)[:, None]
    err = np.abs(u - tg.astype(np.float64))
    tol = slack + TERM_ATOL + TERM_RTOL * np.abs(u)
    print(f"{dec}: max |du| {err.max():.3e}, max err / tol {(err / tol).max():.3e}")
    assert (err <= tol).all()


# ------------------------------------------------------------------- 6. engine and CLI
def _sample_inducer(dev, dec, **kw):
    import torch
    from _profile_sample import sample_data
    data, gold = sample_data()
    ind = _inducer(data, gold, dev, dec, 6, 10, 5, 50, epochs=1, **kw)
    ind.learn(verbose=False)
    torch.cuda.synchronize()
    return data, gold, ind


@pytest.mark.parametrize("dec", DECODERS)
def test_engine_relation_scores_and_top_relations(built_lib, cuda_dev, dec):
    import torch
    from rae.evaluation import relation_scores
    from test_gpu_topk import _snap, _unchanged
    data, _, ind = _sample_inducer(cuda_dev, dec)
    eng = ind.engine
    s0 = _snap(ind)
    n = data.get_arg_voc_size()
    g = np.random.RandomState(1)
    e1, e2 = g.randint(0, n, 77), g.randint(0, n, 77)
    psi = eng.relation_scores(e1, e2)
    torch.cuda.synchronize()
    p64 = _params(ind)
    want = relation_scores(p64, dec, e1, e2)
    bound = psi_bound(dec, p64, e1, e2)
    assert psi.shape == (77, 6) and (np.abs(psi.cpu().numpy() - want) <= bound).all()
    psi2, vals, rel = eng.top_relations(torch.as_tensor(e1), torch.as_tensor(e2), top=3)
    tv, tr = torch.topk(psi2, 3, dim=1)
    assert torch.equal(vals, tv) and torch.equal(rel, tr) and vals.shape == (77, 3)
    assert eng.relation_scores([], []).shape == (0, 6)
    with pytest.raises(IndexError):
        eng.relation_scores([0, n], [0, 0])
    with pytest.raises(IndexError):
        eng.relation_scores([0], [-1])
    assert _unchanged(s0, _snap(ind))


def test_engine_labels_and_cluster_metrics_under_label_with(built_lib, cuda_dev):
    import torch
    from rae.evaluation import GoldIndex, b3_from_table, contingency_table
    from test_gpu_topk import _snap, _unchanged
    data, gold, ind = _sample_inducer(cuda_dev, "rescal+sp")
    eng, ds = ind.engine, ind.engine.split
    s0 = _snap(ind)
    N = ds.N
    enc = eng.label_relations(ds, 0, N, "encoder")
    assert torch.equal(enc, eng.label(ds, 0, N, probs=False)[0])
    psi, joint, ld, lj = eng.eval_relations(ds, 0, N)
    assert torch.equal(eng.label_relations(ds, 0, N, "decoder"), ld)
    assert torch.equal(eng.label_relations(ds, 5, N - 9, "joint"), lj[5:N - 4])
    with pytest.raises(ValueError):
        eng.label_relations(ds, 0, N, "both")
    gi = GoldIndex(gold.get("train", {}), N)
    default = eng.cluster_metrics(ds, gi, 0, N)
    table_enc = contingency_table(enc.cpu().numpy(), gi, 6)
    eng.label_with = "joint"
    try:
        res = eng.cluster_metrics(ds, gi, 0, N, table=True)
    finally:
        eng.label_with = "encoder"
    table = contingency_table(lj.cpu().numpy(), gi, 6)
    assert np.array_equal(res.table, table)
    f1, pre, rec = b3_from_table(table, gi.sizes, gi.n_assessable)[:3]
    assert (res.f1, res.precision, res.recall) == pytest.approx((f1, pre, rec), rel=1e-12)
    again = eng.cluster_metrics(ds, gi, 0, N, table=True)              # the default is untouched
    assert np.array_equal(again.table, table_enc) and again.f1 == default.f1
    assert _unchanged(s0, _snap(ind))


def _cli(tmp_path, extra):
    from _profile_sample import SAMPLE
    from rae import preprocess as P
    plain, out = str(tmp_path / "data-sample.txt"), str(tmp_path / "ds.json.gz")
    if not os.path.exists(out):
        with gzip.open(SAMPLE, "rb") as src, open(plain, "wb") as dst:
            shutil.copyfileobj(src, dst)
        P.preprocess(plain, out)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "rae", out, "--model-name", "m", "--decoder", "rescal+sp",
           "--relations", "6", "--epochs", "2", "--embed-size", "10", "--neg-samples", "5",
           "--batch-size", "50"] + extra
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_cli_label_with_joint_and_predict_relations(built_lib, cuda_dev, tmp_path):
    """One run in a fresh process: joint labels on the device evaluation, three prediction lines;
    and a default run prints what a run without the feature's flags prints."""
    text = _cli(tmp_path, ["--label-with", "joint", "--cluster-eval", "device",
                           "--predict-relations", "3", "--predict-top", "2"])
    lines = text.splitlines()
    assert sum(ln.startswith("train f1: ") for ln in lines) == 2
    assert lines.count("train relations (3 rows)") == 1
    pred = [ln.split("\t") for ln in lines if ln.startswith("relations\t")]
    assert len(pred) == 3
    for i, f in enumerate(pred):
        assert f[1] == str(i) and len(f) == 9 and f[7] == "joint" and 0 <= int(f[8]) < 6
        k, pk = f[4].split(":")
        assert 0 <= int(k) < 6 and 0.0 < float(pk) <= 1.0
        top = [x.split(":") for x in f[5:7]]
        assert all(0 <= int(a) < 6 for a, _ in top) and float(top[0][1]) >= float(top[1][1])


def test_cli_default_output_is_unchanged_by_the_flags_defaults(built_lib, cuda_dev, tmp_path):
    a = _cli(tmp_path, ["--cluster-eval", "device"])
    b = _cli(tmp_path, ["--cluster-eval", "device", "--label-with", "encoder",
                        "--predict-relations", "0"])
    strip = lambda t: [ln for ln in t.splitlines() if "duration" not in ln]
    assert strip(a) == strip(b) and not any(ln.startswith("relations") for ln in strip(a))
