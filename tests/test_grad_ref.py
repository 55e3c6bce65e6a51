"""The host references of tests/_grad_ref.py, on the CPU: the two float64 derivations of one
step's gradients agree under every option, the extraction of a gradient from the state an
AdaGrad step leaves round-trips, and the tolerances of tests/test_gpu_options.py reject each of
a list of planted errors using the host references alone; the checker the GPU tests share
(_grad_ref._check_step) reports a data-parallel plan's dense gradients taken over l instead of
L, under both optimisers, and nothing for the unscaled state.  The saturated regime: the pairwise
softmax backward against np.longdouble and against the oracle's default form, the planted errors
rejected at KAPPA (and not at KAPPA / 2), both float32 hosts finite and the inputs underflowing
exp; the limit shapes U1-U8: row classes, and what plan_resolve decides for each (tests/plan_dump.hip),
U3's s at the LDS edge."""
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


def _caught(ref, bad, kappa=0.0):
    """Tensors on which a planted gradient set exceeds the GPU test's tolerance."""
    return [k for k in ref["g64"]
            if G.rho(bad[k], ref["g64"][k], kappa) > G.tolerance(ref["rho32"][k])]


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
        if c["regime"] == "saturated":
            # a saturated example's dS is nearly zero and its absence shows nowhere: take the
            # row's example with the smallest top-2 logit gap
            S = np.sort(O.encoder_forward(X.astype(np.float64), p["W"][:-1], p["Wb"])[0], axis=1)
            users = coo.row[coo.col == row]
            ex = int(users[np.argmin((S[:, -1] - S[:, -2])[users])])
        col = np.where((coo.col == row) & (coo.row == ex), d, coo.col)
        X = sp.csr_matrix((coo.data, (coo.row, col)), shape=(X.shape[0], d + 1))
    res = O.train_step_grads(c["dec"], p, X.astype(np.float64), e1, e2, n1, n2, alpha=c["alpha"],
                             lambda1=c["l1"], lambda2=c["l2"], adjust=c["l"] / c["N"],
                             ext_reg=c["ext_reg"], softmax_backward=G.softmax_form(c))
    g = dict(res.grads)
    for k in ("A", "Ab") if table == "A" else ("W",):
        g[k] = g[k][:-1]
    return g, row


SAT_PLANTED = ("S1", "S3", "B2", "H1")     # (X1 / X2's heavy row: the sign rule, generic list)
PLANTED = [(s, "O1", "generic") for s in ("S1", "S3", "B2", "H1", "X2")] + \
          [(s, o, "saturated") for s in SAT_PLANTED for o in ("O1", "O3")]


def _pid(shape, option, regime):
    return shape if regime == "generic" else f"{shape}-{option}-sat"


@pytest.mark.parametrize("shape,option,regime", PLANTED, ids=[_pid(*v) for v in PLANTED])
def test_tolerances_reject_planted_errors(shape, option, regime):
    """Teeth: with the tolerance rho <= 16 max(rho_host32, 2^-20) (and COST_RTOL on the cost) each
    planted error shows on at least one tensor, judged from the host references alone.  In the
    saturated regime rho has the KAPPA floor and rho_host32 is the better of the two float32
    hosts; the same list must be rejected under O1 and, less the regulariser's items, under O3,
    where no L2 term hides the small rows of W (it is O3 that decides KAPPA).  One item differs
    there: the example missing from the heaviest W row is the row's least saturated one
    (_duplicate_record), the instance of that error that is easiest to see -- a saturated
    example's dS is nearly zero, so its absence is invisible to this check, and KAPPA is
    certified against the visible instance only."""
    _planted_errors(G.case_config(shape, option, regime=regime))


def test_kappa_is_the_smallest_that_rejects():
    """KAPPA / 2 lets a planted error through on some saturated case of the list above."""
    passed = []
    for shape, option, regime in PLANTED:
        if regime == "saturated" and option == "O3":
            c = G.case_config(shape, option, regime=regime)
            c["kappa"] = G.KAPPA / 2
            try:
                _planted_errors(c)
                passed.append(shape)
            except AssertionError:
                pass
    assert len(passed) < len(SAT_PLANTED), passed


def _planted_errors(c):
    b = 1               # O1: lambda1, lambda2, ext_reg, alpha = 0.1, values; O3: alpha, values
    reg = c["l1"] != 0.0 or c["l2"] != 0.0
    kappa = c["kappa"]
    _caught = lambda ref, bad: globals()["_caught"](ref, bad, kappa)
    ref = G.references(c, b)
    g64 = ref["g64"]
    p = G._p64(c)
    adjust = c["l"] / c["N"]
    assert not _caught(ref, g64)
    if c["regime"] == "saturated":          # each tensor's better float32 host passes
        for k in g64:
            best = ref["g32"] if ref["rho32a"][k] <= ref["rho32c"][k] else ref["g32c"]
            assert G.rho(best[k], g64[k], kappa) <= G.tolerance(ref["rho32"][k]), k
    else:
        assert not _caught(ref, ref["g32"])
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
    for term in (lambda w: c["l2"] * adjust * w, lambda w: c["l1"] * adjust * np.sign(w)) if reg else ():
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
    for k in O.reg_names(c["dec"], c["ext_reg"]) if reg else ():
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
                             ext_reg=c["ext_reg"], softmax_backward=G.softmax_form(c))
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


# --------------------------------------------------------------------------------------------
# the saturated regime: the truth of dS, the two float32 hosts, the inputs
# --------------------------------------------------------------------------------------------
def _softmax_inputs(c, b):
    """(S, d, ce) of batch b in float64: the logits, the decoder's d cost / d P and the entropy
    coefficient 2 alpha / D that the softmax backward takes."""
    X, e1, e2, n1, n2 = G._batch(c, b)
    p = G._p64(c)
    S, P, _ = O.encoder_forward(X.astype(np.float64), p["W"], p["Wb"])
    D = 4 * c["l"] + 2 * c["l"] * c["s"]
    d = O._decoder_forward_backward(c["dec"], p, P, None, e1.astype(np.int64), e2.astype(np.int64),
                                    n1.astype(np.int64), n2.astype(np.int64), D)[2]
    return S, d, 2.0 * c["alpha"] / D


@pytest.mark.parametrize("regime", ["generic", "saturated"])
@pytest.mark.parametrize("shape", ["S3", "S2"])
def test_pairwise_softmax_backward_vs_extended_precision(shape, regime):
    """rae_oracle.softmax_backward_pairwise in float64 against the same form in np.longdouble
    (64-bit significand here) from the same float64 inputs: within 1e-13 of each example's
    rowmax |dS|, every batch; and it is the form the saturated references take."""
    assert np.finfo(np.longdouble).nmant >= 63
    c = G.case_config(shape, "O3", regime=regime)
    assert G.softmax_form(c) == ("pairwise" if regime == "saturated" else "direct")
    for b in range(G.N_BATCHES):
        S, d, ce = _softmax_inputs(c, b)
        got = O.softmax_backward_pairwise(S, d, ce)
        want = O.softmax_backward_pairwise(S.astype(np.longdouble), d.astype(np.longdouble), ce)
        assert want.dtype == np.longdouble
        err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
        assert err.max() <= 1e-13, (b, float(err.max()))


@pytest.mark.parametrize("shape", ["S3", "S2", "B2", "H1", "U2"])
def test_pairwise_equals_direct_softmax_backward_at_generic_parameters(shape):
    """The optional pairwise path against the oracle's default at generic parameters: W and Wb
    within 1e-11 in rho, everything else and the cost bit-identical (the default path is
    unchanged: tests/test_oracle.py and the golden vectors hold it)."""
    c = G.case_config(shape, "O1")
    for b in range(G.N_BATCHES):
        cost, g = G.oracle_step(c, b)
        cost_p, g_p = G.oracle_step(c, b, softmax_backward="pairwise")
        assert cost == cost_p
        for k in g:
            if k in ("W", "Wb"):
                assert G.rho(g_p[k], g[k]) <= 1e-11, (b, k, G.rho(g_p[k], g[k]))
            else:
                assert np.array_equal(g_p[k], g[k]), k


def test_centred_float32_host_is_float32_and_agrees_at_generic_parameters():
    """The second float32 yardstick (the oracle's step in numpy float32 with the centred softmax
    backward) computes in float32 throughout and, at generic parameters, is a float32 host like
    autograd's: within 16 max(rho_host32, 2^-20) of float64 on every tensor."""
    c = G.case_config("S3", "O1")
    ref = G.references(c, 0)
    cost, g = G.centred32_step(c, 0)
    assert abs(cost - ref["cost64"]) <= COST_RTOL * abs(ref["cost64"])
    assert not _caught(ref, g)


SAT_REF_CASES = [(s, o, "saturated") for s, o in G.SAT_CASES] + \
                [(s, o, "saturated-scores") for s, o in G.SAT_SCORE_CASES]


@pytest.mark.parametrize("shape,option,regime", SAT_REF_CASES,
                         ids=[f"{s}-{o}" + ("-scores" if r != "saturated" else "")
                              for s, o, r in SAT_REF_CASES])
def test_saturated_references(shape, option, regime):
    """What the GPU test relies on in the saturated regime, from the host references alone, every
    batch: both float32 hosts finite and their cost within COST_RTOL of float64; at the x 8
    shapes some shifted logit is below -87.3 (fp32 exp underflows); at A, Ab x 2 no decoder
    score reaches +-87 (max |u| is 10 ... 20: printed, not asserted), in the "saturated-scores"
    variant (A, Ab x 32) every batch has scores beyond +-87 and more beyond 16.6 (asserted);
    every gradient element whose square leaves float32's normal range (|g| < 2^-63; the share
    is printed and is NOT below 5 % -- up to 84 % of W without a regulariser, whole columns of a
    one-hot P) lies below what rho_kappa resolves, 2^-20 KAPPA max |g|, so comparing its
    magnitude only loses nothing (at A, Ab x 2 the share does stay under 5 % on A, Ab and the
    hybrid's C, asserted); the
    yardstick is not vacuous: min(autograd32, centred32) <= 2^-7 / 16 on every tensor but W,
    which the planted-error list covers at its own shapes (A, Ab x 2 only: with the scores
    saturated the hybrid's A is 1.5e-3 from float64 on both hosts)."""
    c = G.case_config(shape, option, regime=regime)
    assert c["regime"] == "saturated" and c["scores"] == (regime == "saturated-scores")
    assert c["kappa"] == G.KAPPA and c["ascale"] == (32.0 if c["scores"] else 2.0)
    assert c["wscale"] == (3.0 if shape in ("S1", "B1", "B4") else 8.0)
    p, q = G.generic_params(c), G.generic_params(G.case_config(shape, option))
    assert np.array_equal(p["W"], q["W"] * np.float32(c["wscale"])) and p["W"].dtype == np.float32
    assert np.array_equal(p["A"], q["A"] * np.float32(c["ascale"]))
    assert all(np.array_equal(p[k], q[k]) for k in p if k not in ("W", "Wb", "A", "Ab"))
    for b in range(G.N_BATCHES):
        ref = G.references(c, b)
        st = ref["sat"]
        print(f"SAT {shape}-{option} b{b} |u|>87 {st['u']:.4f} |u|>16.6 {st['u16']:.4f} "
              f"z<-87.3 {st['z']:.4f} gap {st['gap']:.1f}")
        assert st["gap"] > 40.0
        if c["scores"]:
            assert st["u"] > 0.0 and st["u16"] > st["u"], (b, st)
        if c["wscale"] == 8.0:
            assert st["z"] > 0.0, b
        for cost in (ref["cost32"], ref["cost32c"]):
            assert abs(cost - ref["cost64"]) <= COST_RTOL * max(1.0, abs(ref["cost64"])), b
        for k, g64 in ref["g64"].items():
            assert np.all(np.isfinite(ref["g32"][k])) and np.all(np.isfinite(ref["g32c"][k])), k
            print(f"YARD {shape}-{option} b{b} {k:2s} autograd32 {ref['rho32a'][k]:.3e} "
                  f"centred32 {ref['rho32c'][k]:.3e} underflow {G.underflow_share(g64):.4f}")
            a64 = np.abs(g64)
            small = (a64 > 0.0) & (a64 < G.G2_MIN)
            assert np.all(a64[small] < G.FLOOR * G.KAPPA * a64.max()), (b, k)
            if not c["scores"] and k in ("A", "Ab", "C"):
                assert G.underflow_share(g64) < 0.05, (b, k)
            if k != "W" and not c["scores"]:     # (scores: A of H1 is 1.5e-3 from float64)
                assert ref["rho32"][k] <= 2.0 ** -7 / G.FACTOR, (b, k, ref["rho32"][k])


# --------------------------------------------------------------------------------------------
# the limit shapes U1-U8
# --------------------------------------------------------------------------------------------
from test_plan import plan_dump     # noqa: E402,F401  (the host-only plan_resolve dump, a fixture)


def _resolve(plan_dump, c, **extra):
    import subprocess
    data, _, _ = G.case_dataset(c)
    X = data.split["train"].xFeats
    nnz = np.diff(X.indptr)
    cfg = dict(decoder=O.DECODERS.index(c["dec"]), optimizer=0 if c["opt"] == "adagrad" else 1,
               n_examples=c["N"], n_features=c["d"], n_entities=c["n"], relations=c["m"],
               embed=c["r"], neg_samples=c["s"], batch_size=c["l"], world_size=1, rank=0,
               learning_rate=c["lr"], alpha=c["alpha"], lambda1=c["l1"], lambda2=c["l2"],
               ext_reg=int(c["ext_reg"]), max_row_nnz=int(nnz.max()),
               max_batch_nnz=int(max(nnz[b * c["l"]:(b + 1) * c["l"]].sum()
                                     for b in range(G.N_BATCHES))),
               neg_stride=c["N"], mfma_bf16=int(c["bf16"]))
    cfg.update(extra)
    out = subprocess.run([plan_dump, *[f"{k}={v}" for k, v in cfg.items()]], capture_output=True,
                         text=True, check=True).stdout.splitlines()
    return dict(line.split(" ", 1) for line in out)


LDS_MESSAGE = "configuration needs more than 160 KiB LDS per example workgroup"


def test_limit_shapes_resolve_at_the_edges(plan_dump):
    """plan_resolve on the U shapes (host only): every one is accepted; U1 and U3 take the split
    SP forward and U2 the fused one; the scalar shapes resolve to v4 = 0 with two elements per
    lane (q = 2) and the 512 shapes to float4 rows with q = 2; U3's s is the largest accepted at
    m = r = 512 -- one more is rejected with the LDS message, and its fused example workgroup
    would sit within 3 KiB of the 160 KiB limit; the hybrid U8 is within 16 KiB."""
    want = {"U1": ("1", "2", "1"), "U2": ("0", "2", "0"), "U3": ("1", "2", "1"),
            "U3f": ("1", "2", "0"),
            "U4": ("1", "2", "0"), "U5": ("0", "2", "0"), "U6": ("0", "2", "0"),
            "U7": ("1", "2", "0"), "U8": ("1", "2", "0")}
    assert tuple(want) == G.LIMIT_SHAPES
    for shape, (v4, q, split) in want.items():
        for option in ("O1", "O3"):
            c = G.case_config(shape, option)
            d = _resolve(plan_dump, c, sp_forward={"fused": 1, "split": 2}.get(
                c["forms"].get("sp_forward"), 0))
            assert d["rc"] == "0", (shape, d)
            assert (d["v4"], d["q"], d["sp_split"]) == (v4, q, split), (shape, option)
            assert int(d["smem_fwd"]) <= 160 * 1024
    c = G.case_config("U3", "O3")
    assert c["s"] == G.U3_SMAX and (c["m"], c["r"]) == (512, 512)
    d = _resolve(plan_dump, c)
    assert 157 * 1024 < int(d["smem_fwd"]) <= 160 * 1024, d["smem_fwd"]
    over = _resolve(plan_dump, c, neg_samples=c["s"] + 1)
    assert over["rc"] != "0" and over["err"].startswith(LDS_MESSAGE), over
    assert _resolve(plan_dump, G.case_config("U1", "O3"), neg_samples=50)["err"].startswith(LDS_MESSAGE)
    d = _resolve(plan_dump, G.case_config("U7", "O3"))
    assert (d["bf16"], d["mt_bf16"], d["mt_direct"]) == ("1", "0", "1")     # m > 128: fp32 M


def test_limit_shape_datasets_hold_every_row_class():
    """Every batch of every U shape's dataset (l = 32 or 40, n = 4000, 600 <= d <= 1500) holds
    every row class of both tables; the columns are what the issue of each shape needs."""
    for shape in G.LIMIT_SHAPES:
        for option in ("O1", "O3"):
            c = G.case_config(shape, option)
            assert (shape, option) in G.CASES and c["n"] == 4000 and 600 <= c["d"] <= 1500
            data, n1, n2 = G.case_dataset(c)
            for b in range(G.N_BATCHES):
                ca, cw = G.batch_row_classes(data, n1, n2, c["l"], b)
                assert min(G._class_counts(ca)) > 0 and min(G._class_counts(cw)) > 0, (shape, b)
    for shape in ("U2", "U5", "U6"):        # scalar rows, two elements per lane
        c = G.case_config(shape, "O3")
        assert 64 < c["m"] <= 128 and (c["m"] % 4 or c["r"] % 4)
    assert G.case_config("U2", "O3")["r"] == 125
    dp = {G.dp_case_id(case) for case in G.DP_CASES}
    assert {"U1-O3-G2-partials", "U2-O3-G2-records", "U4-O3-G2"} <= dp
