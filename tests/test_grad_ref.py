"""The host references of tests/_grad_ref.py, on the CPU: the two float64 derivations of one
step's gradients agree under every option, the extraction of a gradient from the state an
AdaGrad step leaves round-trips, and the tolerances of tests/test_gpu_options.py reject each of
a list of planted errors using the host references alone; the checker the GPU tests share
(_grad_ref._check_step) reports a data-parallel plan's dense gradients taken over l instead of
L, under both optimisers, and nothing for the unscaled state."""
import numpy as np
import pytest
import scipy.sparse as sp

import _grad_ref as G
import rae_oracle as O

COST_RTOL = 2e-5            # tests/test_gpu_train.py


@pytest.mark.parametrize("shape,option", G.CASES, ids=[f"{s}-{o}" for s, o in G.CASES])
def test_two_float64_derivations_agree(shape, option):
    """The analytic oracle against float64 autograd of cpu_ref.cost_graph (+ the regulariser),
    every batch of every case of test_gpu_options.py, feature values and regulariser included."""
    c = G.case_config(shape, option)
    for b in range(G.N_BATCHES):
        cost, g = G.oracle_step(c, b)
        cost_a, g_a = G.autograd_step(c, b)
        assert abs(cost - cost_a) <= 1e-11 * max(1.0, abs(cost)), (b, cost, cost_a)
        for k in g:
            assert np.all(np.isfinite(g[k])), k
            assert G.rho(g_a[k], g[k]) <= 1e-11, (b, k, G.rho(g_a[k], g[k]))


def test_datasets_hold_every_row_class():
    """Every batch of every dataset the cases use has rows of both tables with exactly 1 record,
    2-4, 5-16 and more than 16 (options_dataset asserts it; the counts at C3's shape are pinned
    here), and the hot variant a row of at least 256 records."""
    for shape, option in G.CASES:
        G.case_dataset(G.case_config(shape, option))
    c = G.case_config("S1", "O0")
    data, n1, n2 = G.case_dataset(c)
    ca, _ = G.batch_row_classes(data, n1, n2, c["l"], 0)
    assert G._class_counts(ca) == [2212, 326, 64, 13]
    c = G.case_config("X1", "O1")
    data, n1, n2 = G.case_dataset(c)
    for b in range(G.N_BATCHES):
        assert G.batch_row_classes(data, n1, n2, c["l"], b)[0].max() >= 256


@pytest.mark.parametrize("shape", ["S3", "B2", "H1"])
def test_adagrad_extraction_round_trips(shape):
    """opt_update emulated in numpy float32 on the rounded oracle gradient, then the extraction
    the GPU test applies to the device's state: the gradient comes back within 2^-23."""
    c = G.case_config(shape, "O1")
    ref = G.references(c, 0)
    p0 = G.generic_params(c)
    for k, g64 in ref["g64"].items():
        g = g64.astype(np.float32)
        p1, acc = G.emulate_opt_update(p0[k], np.zeros_like(p0[k]), g, c["lr"], "adagrad")
        got = G.extract_adagrad(p0[k], p1, acc, g64, G.tolerance(ref["rho32"][k]))
        assert G.rho(got, g.astype(np.float64)) <= 2.0 ** -23, k
        # the step the GPU test predicts from the extracted gradient
        root = np.sqrt(acc.astype(np.float64))
        off = np.abs(np.abs(p0[k].astype(np.float64) - p1) - c["lr"] * root / (root + 1e-6))
        assert np.all(off <= 8 * 2.0 ** -24 * (np.abs(p0[k]) + c["lr"])), k
        # SGD: one rounding of p - lr g
        p1s, _ = G.emulate_opt_update(p0[k], np.zeros_like(p0[k]), g, 1.0, "sgd")
        assert np.all(np.abs(p1s - (p0[k].astype(np.float64) - g64)) <=
                      2.0 ** -23 * np.abs(p1s) + 2.0 ** -23 * np.abs(g64)), k


def _caught(ref, bad):
    """Tensors on which a planted gradient set exceeds the GPU test's tolerance."""
    return [k for k in ref["g64"]
            if G.rho(bad[k], ref["g64"][k]) > G.tolerance(ref["rho32"][k])]


def _cost_caught(ref, cost):
    return abs(cost - ref["cost64"]) > COST_RTOL * max(1.0, abs(ref["cost64"]))


def _duplicate_record(c, b, table):
    """The oracle's gradients with ONE example's contribution to the heaviest row of `table`
    removed: the record is pointed at a fresh copy of the row (same values, so the forward and
    every other gradient are unchanged) and the copy's gradient is dropped."""
    X, e1, e2, n1, n2 = G._batch(c, b)
    p = G._p64(c)
    if table == "A":
        ids = np.concatenate([e1, e2, n1.ravel(), n2.ravel()])
        row = int(np.bincount(ids).argmax())
        n = p["A"].shape[0]
        p["A"] = np.vstack([p["A"], p["A"][row:row + 1]])
        p["Ab"] = np.concatenate([p["Ab"], p["Ab"][row:row + 1]])
        e1, e2, n1, n2 = (a.copy() for a in (e1, e2, n1, n2))
        ex = next(j for j in range(c["l"]) if row in (e1[j], e2[j], *n1[:, j], *n2[:, j]))
        for a in (e1, e2):
            if a[ex] == row:
                a[ex] = n
        for a in (n1, n2):
            a[a[:, ex] == row, ex] = n
    else:
        X = sp.csr_matrix(X)
        row = int(np.bincount(X.indices).argmax())
        d = X.shape[1]
        p["W"] = np.vstack([p["W"], p["W"][row:row + 1]])
        coo = X.tocoo()
        ex = int(coo.row[coo.col == row][0])
        col = np.where((coo.col == row) & (coo.row == ex), d, coo.col)
        X = sp.csr_matrix((coo.data, (coo.row, col)), shape=(X.shape[0], d + 1))
    res = O.train_step_grads(c["dec"], p, X.astype(np.float64), e1, e2, n1, n2, alpha=c["alpha"],
                             lambda1=c["l1"], lambda2=c["l2"], adjust=c["l"] / c["N"],
                             ext_reg=c["ext_reg"])
    g = dict(res.grads)
    for k in ("A", "Ab") if table == "A" else ("W",):
        g[k] = g[k][:-1]
    return g, row


@pytest.mark.parametrize("shape", ["S1", "S3", "B2", "H1", "X2"])
def test_tolerances_reject_planted_errors(shape):
    """Teeth: with the tolerance rho <= 16 max(rho_host32, 2^-20) (and COST_RTOL on the cost) each
    planted error shows on at least one tensor, judged from the host references alone."""
    c = G.case_config(shape, "O1")          # lambda1, lambda2, ext_reg, alpha = 0.1, values
    b = 1
    ref = G.references(c, b)
    g64 = ref["g64"]
    p = G._p64(c)
    adjust = c["l"] / c["N"]
    assert not _caught(ref, g64) and not _caught(ref, ref["g32"])
    # one tensor's gradient scaled by 1 + 2^-7: each tensor in turn
    for k in g64:
        bad = dict(g64)
        bad[k] = g64[k] * (1.0 + 2.0 ** -7)
        assert _caught(ref, bad) == [k]
    # one example's contribution missing from the heaviest A row / W row
    for table in ("A", "W"):
        bad, row = _duplicate_record(c, b, table)
        hit = _caught(ref, bad)
        assert table in hit, (table, row, hit)
        others = [k for k in g64 if k not in (("A", "Ab") if table == "A" else ("W",))]
        assert not set(hit) & set(others), hit      # ... and nothing else moved
    # alpha off by 1 %
    assert _caught(ref, G.oracle_step(c, b, alpha=c["alpha"] * 1.01)[1])
    # lambda2 applied as lambda2 instead of 2 lambda2; sgn(w) dropped
    for term in (lambda w: c["l2"] * adjust * w, lambda w: c["l1"] * adjust * np.sign(w)):
        bad = dict(g64)
        for k in O.reg_names(c["dec"], c["ext_reg"]):
            bad[k] = g64[k] - term(p[k])
        assert sorted(_caught(ref, bad)) == sorted(O.reg_names(c["dec"], c["ext_reg"]))
    # one tile's L1 / L2 partial left out of the cost: a 16 x 16 tile of C1, 16 rows (i, j) of
    # R / C, one block's share of the dense W sweep (1 / 1024 of W)
    tiles = {"C1": lambda w: w[:16, :16], "C2": lambda w: w[:16, :16],
             "R": lambda w: w.reshape(-1, w.shape[-1])[:16],
             "C": lambda w: w.reshape(-1, w.shape[-1])[:16],
             "W": lambda w: w.ravel()[:max(1, w.size // 1024)]}
    for k in O.reg_names(c["dec"], c["ext_reg"]):
        t = tiles[k](p[k])
        part = adjust * (c["l1"] * np.abs(t).sum() + c["l2"] * np.square(t).sum())
        assert _cost_caught(ref, ref["cost64"] - part), (k, part, ref["cost64"])
    assert not _cost_caught(ref, ref["cost32"])
    # feature values treated as 1
    X, e1, e2, n1, n2 = G._batch(c, b)
    ones = sp.csr_matrix((np.ones_like(X.data, dtype=np.float64), X.indices, X.indptr),
                         shape=X.shape)
    res = O.train_step_grads(c["dec"], p, ones, e1, e2, n1, n2, alpha=c["alpha"],
                             lambda1=c["l1"], lambda2=c["l2"], adjust=adjust,
                             ext_reg=c["ext_reg"])
    assert "W" in _caught(ref, res.grads)


# --------------------------------------------------------------------------------------------
# the data-parallel cases (tests/test_gpu_dp_options.py)
# --------------------------------------------------------------------------------------------
def test_dp_datasets_hold_every_row_class():
    """Every batch of every data-parallel case's dataset holds every row class of both tables
    (options_dataset asserts it; the new L = 36 set is looked at here batch by batch), the hot
    sets a row of at least 256 records; the global batch divides into the ranks, and no
    partitioned case carries a regulariser (plan_resolve refuses the pair)."""
    for case in G.DP_CASES:
        shape, option, ranks, dense, priv, part = case
        c = G.dp_case_config(shape, option)
        data, n1, n2 = G.case_dataset(c)
        assert c["l"] % ranks == 0 and data.split["train"].args1.shape[0] == G.N_BATCHES * c["l"]
        assert not (part and (c["l1"] != 0.0 or c["l2"] != 0.0)), case
        assert dense is None or c["dec"] == "sp", case
        if c["hot"]:
            for b in range(G.N_BATCHES):
                assert G.batch_row_classes(data, n1, n2, c["l"], b)[0].max() >= 256
    assert len({G.dp_case_id(case) for case in G.DP_CASES}) == len(G.DP_CASES)
    c = G.dp_case_config("S4p", "O1")
    assert (c["l"], c["n"], c["d"]) == (36, 4000, 500)
    data, n1, n2 = G.case_dataset(c)
    for b in range(G.N_BATCHES):
        ca, cw = G.batch_row_classes(data, n1, n2, c["l"], b)
        assert min(G._class_counts(ca)) > 0 and min(G._class_counts(cw)) > 0, b
    assert G.SHAPES.keys() == G.DP_SHAPES.keys() - {"S4p"}
    assert all(G.DP_SHAPES[k] is G.SHAPES[k] for k in G.SHAPES)


def _state_of(c, b, scale):
    """The state a device that computed the float32 host gradient -- tensor k's times
    scale.get(k, 1) -- would leave after batch b: (cost, p1, acc), by opt_update in float32."""
    ref = G.references(c, b)
    p0 = G.generic_params(c)
    p1, acc = {}, {}
    for k, g in ref["g32"].items():
        g = (g * scale.get(k, 1.0)).astype(np.float32)
        p1[k], a = G.emulate_opt_update(p0[k], np.zeros_like(p0[k]), g, c["lr"], c["opt"])
        if c["opt"] == "adagrad":
            acc[k] = a
    return ref["cost32"], p1, acc


def _reported(bad):
    """The tensors (or "cost") _check_step's failure lines name."""
    return sorted({line.split()[1].rstrip(":") for line in bad})


@pytest.mark.parametrize("option", ["O3", "O0"])
def test_checker_reports_dense_gradients_over_l_instead_of_L(option):
    """What the data-parallel tests exist to catch: the dense tensors' gradient (C1, C2, Wb) of
    a 2-rank plan normalised by l instead of L, i.e. scaled by l / L = 1 / 2.  AdaGrad's step is
    invariant to such a factor up to its epsilon (lr g / (|g| + 1e-6) from a zero accumulator), so
    the parameters hardly tell; _check_step reads |g| from sqrt(acc) and reports exactly those
    tensors, as it does under SGD from p0 - p1.  The unscaled float32 host state passes."""
    c = G.case_config("S1", option)
    assert c["opt"] == ("sgd" if option == "O3" else "adagrad")
    dense = {"C1": 0.5, "C2": 0.5, "Wb": 0.5}
    for b in range(G.N_BATCHES):
        bad = []
        G._check_step(c, b, *_state_of(c, b, {}), f"host32-{option}", bad)
        assert bad == []
        G._check_step(c, b, *_state_of(c, b, dense), f"halved-{option}", bad)
        assert _reported(bad) == sorted(dense), bad
