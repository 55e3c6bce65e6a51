"""Host references for one training step under every optimiser / regulariser option
(tests/test_grad_ref.py pins them on the CPU; tests/test_gpu_options.py holds the device to them at
one rank, tests/test_gpu_dp_options.py the data-parallel forms at the same global batch).

* a dataset whose batches hold every row class of the update (rows of the A and of the W table
  with exactly 1 record, 2-4, 5-16 and more than 16 records), and a "hot" variant with a row
  of at least 256 records (the heavy-row chunks);
* generic parameters (no zero biases, no near-uniform P) in place of the reference
  initialisation;
* three references for the gradients of one step: the analytic float64 oracle
  (rae_oracle.train_step_grads), the same with the bf16 operand rounding emulated, and
  autograd of cpu_ref.cost_graph (float64: a second derivation; float32: the yardstick for
  what single precision costs at these parameters);
* the metric rho and the extraction of the gradient from the device's state after one step;
* the shapes at the upper end of what plan_resolve accepts (U1-U8);
* a "saturated" regime of the same parameters (W, Wb x 8 or x 3, A, Ab x 2: P near one-hot,
  scores past +-87), for which the float64 truth of W / Wb takes the pairwise softmax backward
  (rae_oracle.softmax_backward_pairwise), a second float32 host (the oracle in float32 with
  the device's centred formula) stands beside float32 autograd, and rho floors its
  denominator at KAPPA times the tensor's largest gradient.
"""
import functools
import math
import sys

import numpy as np
import torch

import cpu_ref
import rae_oracle as O

ROW_CLASSES = ((1, 1), (2, 4), (5, 16), (17, 1 << 30))
FLOOR = 2.0 ** -20          # floor of the float32 yardstick
FACTOR = 16.0               # device <= FACTOR * max(host float32, FLOOR), both against float64
LAMBDA1, LAMBDA2 = 0.01, 0.1
# The saturated regime.  rho_kappa divides by max(rowmax|g|, KAPPA max|g| over the tensor): rows of
# W whose true gradient is 1e-22 ... 1e-8 of the tensor's carry absolute float32 noise of the
# softmax backward, which no float32 implementation can hold to their own rowmax.  KAPPA is the
# smallest power of two in 2^-20 ... 2^-8 at which every planted error of
# tests/test_grad_ref.py::test_tolerances_reject_planted_errors is rejected on every tensor
# from the host references alone (test_kappa_is_the_smallest_that_rejects pins it).  "One example
# missing from the heaviest W row" is planted there with the row's LEAST saturated example: a
# saturated example's dS is nearly zero, and its absence is invisible to this check at any KAPPA.
KAPPA = 2.0 ** -10
U_SAT, Z_SAT = 87.0, -87.3      # |score| beyond which sigmoid is 0 / 1 in fp32; exp underflow
U_LIN = 16.6                    # |score| beyond which the kernels' softplus is max(x, 0)
SAT_A = 2.0                     # A, Ab factor
SAT_A_SCORES = 32.0             # ... of the "saturated-scores" variant
SAT_W = {"S1": 3.0, "B1": 3.0, "B4": 3.0}       # W, Wb factor at the C3 / C5 shapes; 8 elsewhere
SAT_W_DEFAULT = 8.0
G2_MIN = 2.0 ** -63             # |g| below it: g^2 is below the smallest normal float32
U3_SMAX = 26                    # the largest s plan_resolve accepts at sp m = r = 512

# option sets: optimiser, lambda1, lambda2, ext_reg, alpha, non-binary feature values, lr
OPTIONS = {
    "O0": dict(opt="adagrad", l1=0.0, l2=0.0, ext_reg=True, alpha=1.0, values=False, lr=0.1),
    "O1": dict(opt="adagrad", l1=LAMBDA1, l2=LAMBDA2, ext_reg=True, alpha=0.1, values=True, lr=0.1),
    "O2": dict(opt="adagrad", l1=LAMBDA1, l2=LAMBDA2, ext_reg=False, alpha=1.0, values=False, lr=0.1),
    "O3": dict(opt="sgd", l1=0.0, l2=0.0, ext_reg=True, alpha=0.1, values=True, lr=1.0),
    "O4": dict(opt="sgd", l1=LAMBDA1, l2=LAMBDA2, ext_reg=True, alpha=1.0, values=False, lr=1.0),
}

# shapes: decoder, (m, r, s, l), d, bf16 operands, kernel forms asked for, forms expected
SHAPES = {
    "S1": dict(dec="sp", mrsl=(100, 200, 20, 100), d=3000, want={"sp_forward": "fused"}),
    "S2": dict(dec="sp", mrsl=(30, 100, 10, 60), d=500, want={"sp_forward": "fused"}),
    "S3": dict(dec="sp", mrsl=(7, 13, 3, 70), d=700, want={"sp_forward": "fused"}),
    "S4": dict(dec="sp", mrsl=(8, 44, 5, 37), d=500, forms={"sp_forward": "split"},
               want={"sp_forward": "split"}),
    "S5": dict(dec="sp", mrsl=(300, 300, 50, 37), d=1500, want={"sp_forward": "split"}),
    "B1": dict(dec="rescal", mrsl=(100, 200, 20, 100), d=2000),
    "B2": dict(dec="rescal", mrsl=(7, 13, 3, 70), d=700),
    "B3": dict(dec="rescal", mrsl=(400, 24, 3, 40), d=600),
    "B4": dict(dec="rescal", mrsl=(100, 200, 20, 100), d=2000, bf16=True),
    "B5": dict(dec="rescal", mrsl=(60, 96, 5, 40), d=800, bf16=True),
    "B6": dict(dec="rescal", mrsl=(132, 24, 3, 40), d=600, bf16=True),
    "H1": dict(dec="rescal+sp", mrsl=(30, 60, 10, 100), d=1000),
    "H2": dict(dec="rescal+sp", mrsl=(7, 13, 3, 70), d=700),
    "H3": dict(dec="rescal+sp", mrsl=(100, 200, 20, 100), d=2000, bf16=True),
    "X1": dict(dec="sp", mrsl=(8, 16, 4, 256), d=300, hot=True, forms={"heavy_chunk": "on"},
               want={"heavy_chunk": "on"}),
    "X2": dict(dec="rescal+sp", mrsl=(8, 16, 4, 256), d=300, hot=True,
               forms={"heavy_chunk": "on"}, want={"heavy_chunk": "on"}),
    # the upper end of the accepted range: 512 (multiples of 4: eight softmax slots per lane of
    # wave 0), 65 ... 128 columns not a multiple of 4 (the scalar paths with two elements per
    # lane), the largest s at m = r = 512 (example_smem_floats just under 160 KiB;
    # tests/test_grad_ref.py holds U3_SMAX to the plan)
    "U1": dict(dec="sp", mrsl=(512, 512, 5, 32), d=1000, want={"sp_forward": "split"}),
    "U2": dict(dec="sp", mrsl=(127, 125, 3, 32), d=700, want={"sp_forward": "fused"}),
    "U3": dict(dec="sp", mrsl=(512, 512, U3_SMAX, 32), d=1000, want={"sp_forward": "split"}),
    # U3 with the fused forward forced: the example workgroup that takes those 161 392 bytes
    "U3f": dict(dec="sp", mrsl=(512, 512, U3_SMAX, 32), d=1000, forms={"sp_forward": "fused"},
                want={"sp_forward": "fused"}),
    "U4": dict(dec="rescal", mrsl=(512, 16, 3, 32), d=600),
    "U5": dict(dec="rescal", mrsl=(127, 31, 3, 32), d=700),
    "U6": dict(dec="rescal+sp", mrsl=(126, 31, 3, 32), d=800),
    "U7": dict(dec="rescal", mrsl=(512, 32, 3, 40), d=600, bf16=True),   # m > 128: fp32 M
    "U8": dict(dec="rescal+sp", mrsl=(508, 36, 3, 32), d=900),
}
LIMIT_SHAPES = tuple(k for k in SHAPES if k.startswith("U"))

ALL_OPTIONS = ("S1", "S3", "B1", "B4", "H1")
CASES = [(sh, op) for sh in SHAPES
         for op in (tuple(OPTIONS) if sh in ALL_OPTIONS else ("O1", "O3"))]
N_BATCHES = 3
# the saturated regime: the same shapes' parameters scaled (case_config(..., regime="saturated"))
SAT_SHAPES = ("S1", "S2", "S3", "S4", "S5", "B1", "B2", "B5", "H1", "X1")
SAT_CASES = [(sh, op) for sh in SAT_SHAPES for op in ("O1", "O3")]
# ... and AdaGrad without a regulariser: O1's L2 term (0.07 |w|) covers the small rows of W and
# O3's SGD step reads a gradient only to an ulp of the parameter (2^-23 |w| / lr, |w| ~ 5 here),
# while sqrt(acc) shows every W row's gradient to one rounding
# (S3 and B2 are left out: with O0's binary features their first batch stops at z = -86.3)
SAT_CASES += [(sh, "O0") for sh in ("S1", "S2", "S4", "S5", "B1", "B5", "H1", "X1")]
# the "saturated-scores" variant: A, Ab x 32 instead of x 2, so that the decoder's scores saturate
# too (at x 2 the largest |u| is 10 ... 20): 8 ... 12 % of the scores of the SP shapes and over
# 90 % of the bilinear ones (u is quadratic in A there) lie beyond +-87, where fp32 sigmoid is
# exactly 0 or 1, and more beyond the 16.6 from which the kernels' softplus is max(x, 0); both
# float32 hosts stay finite (chosen on the CPU: at x 16 no SP batch passes 87)
SAT_SCORE_CASES = [(sh, op) for sh in ("S1", "S3", "B2", "H1") for op in ("O1", "O3")]

# Data-parallel cases (tests/test_gpu_dp_options.py).  A shape's batch is the GLOBAL batch L of
# G ranks with l = L / G examples each, so the references of a case are those of the single-rank
# case at l = L.  DP_SHAPES adds what SHAPES lacks: S4p, the forced split SP forward at L = 36
# (three ranks of 12).
DP_SHAPES = dict(SHAPES)
DP_SHAPES["S4p"] = dict(dec="sp", mrsl=(8, 44, 5, 36), d=500, forms={"sp_forward": "split"},
                        want={"sp_forward": "split"})


def _dp_cases():
    """(shape, option, G, dp_dense, priv_rows, partitioned): dp_dense / priv_rows None leave the
    form to the plan; partitioned cases run the replicated update too (same forms) and compare
    the two bitwise.  A regulariser (O1, O4) goes with the replicated update only."""
    out = []

    def add(shape, option, G, dense=None, priv=None, part=False):
        out.append((shape, option, G, dense, priv, part))
    for G in (2, 4):
        for dense in ("records", "partials"):
            for op in ("O1", "O3", "O4"):
                add("S1", op, G, dense)
    for dense in ("partials", "records"):
        for priv in ("on", "off"):
            for op in ("O0", "O3"):
                add("S1", op, 2, dense, priv, True)
    for G in (2, 5):                        # the scalar path; G = 5: 14 rows owned of L = 70
        for dense in ("records", "partials"):
            for op in ("O1", "O3"):
                add("S3", op, G, dense, None, G == 5 and op == "O3")
    for op in ("O1", "O3"):
        add("S4p", op, 3, "partials")
        add("B1", op, 2, part=op == "O3")
        add("B2", op, 2)
    for op in ("O1", "O3", "O4"):
        add("H1", op, 4, part=op == "O3")
    for op in ("O1", "O3"):
        add("B4", op, 2)
        add("B5", op, 2, part=op == "O3")   # L = 40: Lp = 64 has 24 padding examples
    add("B6", "O3", 2)                      # m > 128
    add("H3", "O3", 2)
    add("U1", "O3", 2, "partials")          # m = r = 512, the split forward
    add("U2", "O3", 2, "records")           # scalar rows, two elements per lane
    add("U4", "O3", 2)                      # bilinear at m = 512
    for shape in ("X1", "X2"):
        add(shape, "O3", 2, part=True)
        add(shape, "O1", 2)
    return out


DP_CASES = _dp_cases()


def dp_case_id(case):
    shape, option, G, dense, priv, part = case
    return (f"{shape}-{option}-G{G}" + (f"-{dense}" if dense else "") +
            (f"-priv_{priv}" if priv else "") + ("-part" if part else ""))


def dp_case_config(shape, option):
    """The global-batch config of a data-parallel case (l is the global batch L)."""
    return case_config(shape, option, DP_SHAPES)


def case_config(shape, option, shapes=None, regime="generic"):
    """Everything one (shape, option) case needs, as a dict.  regime "generic": generic_params as
    drawn; "saturated": W, Wb times SAT_W (8; 3 at the C3 / C5 shapes), A, Ab times SAT_A;
    "saturated-scores": the same with A, Ab times SAT_A_SCORES (c["regime"] is "saturated" for
    both, c["scores"] tells them apart)."""
    assert regime in ("generic", "saturated", "saturated-scores"), regime
    c = dict((shapes or SHAPES)[shape])
    c["scores"] = regime == "saturated-scores"      # ... the decoder's scores saturate as well
    regime = c["regime"] = "generic" if regime == "generic" else "saturated"
    c["kappa"] = KAPPA if regime == "saturated" else 0.0
    c["wscale"] = SAT_W.get(shape, SAT_W_DEFAULT) if regime == "saturated" else 1.0
    c["ascale"] = (SAT_A_SCORES if c["scores"] else SAT_A) if regime == "saturated" else 1.0
    c.update(OPTIONS[option])
    c["m"], c["r"], c["s"], c["l"] = c.pop("mrsl")
    c["n"] = 20000 if (c["l"], c["s"]) == (100, 20) else 4000
    c["N"] = N_BATCHES * c["l"]
    c.setdefault("bf16", False)
    c.setdefault("hot", False)
    c.setdefault("forms", {})
    c.setdefault("want", {})
    c["shape"], c["option"] = shape, option
    return c


# --------------------------------------------------------------------------------------------
# dataset
# --------------------------------------------------------------------------------------------
def _class_counts(counts):
    counts = counts[counts > 0]
    return [int(((counts >= lo) & (counts <= hi)).sum()) for lo, hi in ROW_CLASSES]


def batch_row_classes(data, neg1, neg2, l, b):
    """Rows of the A and of the W table per record-count class in batch b."""
    xs = data.split["train"]
    rows = slice(b * l, (b + 1) * l)
    ids = np.concatenate([xs.args1[rows], xs.args2[rows], neg1[:, rows].ravel(),
                          neg2[:, rows].ravel()])
    ca = np.bincount(ids, minlength=data.get_arg_voc_size())
    cw = np.bincount(xs.xFeats[rows].indices, minlength=data.get_dimensionality())
    return ca, cw


@functools.lru_cache(maxsize=None)
def options_dataset(l, s, n, d, hot=False, values=False):
    """(DatasetManager, neg1, neg2): features of synthetic_dataset(3 l, d, 6, seed=99), entities
    from a Zipf(1.2) vocabulary of n ids of its own, so a batch references most entity rows
    once, some a few times and a few very often -- synthetic_dataset's own n = N / 5 entities
    make every A row of a small batch very heavy.  Every batch holds every row class of both
    tables (asserted).  hot: the first four ids' frequencies are raised until every batch has
    a row of at least 256 records."""
    from rae.data import DatasetManager, DatasetSplit, synthetic_dataset
    N = N_BATCHES * l
    feats, _ = synthetic_dataset(N, d, 6, seed=99)
    X = feats.split["train"].xFeats.copy()
    if values:
        X.data = np.random.RandomState(5).uniform(0.5, 2.0, size=X.data.shape).astype(np.float32)
    base = np.ceil(n / np.power(1.0 + np.arange(n), 1.2)).astype(np.int64)
    boost = 1
    while True:
        freqs = base.copy()
        freqs[:4] *= boost
        g = np.random.RandomState(7)
        p = freqs / freqs.sum()
        a1 = g.choice(n, size=N, p=p).astype(np.int32)
        a2 = g.choice(n, size=N, p=p).astype(np.int32)
        a2[::7] = a1[::7]
        data = DatasetManager({"train": DatasetSplit(a1, a2, X)}, freqs, d)
        gn = np.random.RandomState(2)
        neg1 = O.negative_samples(gn, data.negSamplingCum, N, s)
        neg2 = O.negative_samples(gn, data.negSamplingCum, N, s)
        tops = [batch_row_classes(data, neg1, neg2, l, b)[0].max() for b in range(N_BATCHES)]
        if not hot or min(tops) >= 256:
            break
        boost *= 2
        assert boost <= 1 << 16
    for b in range(N_BATCHES):
        ca, cw = batch_row_classes(data, neg1, neg2, l, b)
        assert min(_class_counts(ca)) > 0, ("A row classes", l, s, b, _class_counts(ca))
        assert min(_class_counts(cw)) > 0, ("W row classes", l, s, b, _class_counts(cw))
        if hot:
            assert ca.max() >= 256, (b, ca.max())
    return data, neg1, neg2


def case_dataset(c):
    return options_dataset(c["l"], c["s"], c["n"], c["d"], c["hot"], c["values"])


# --------------------------------------------------------------------------------------------
# parameters
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic_params(decoder, d, m, n, r):
    g = np.random.RandomState(13)
    shapes = {"W": (d, m), "Wb": (m,), "A": (n, r), "Ab": (n,), "C1": (r, m), "C2": (r, m),
              "R": (r, r, m), "C": (r, r, m)}
    sd = {"W": 0.6, "A": 1.0 / math.sqrt(r)}
    p = {}
    for k in O.param_names(decoder):
        p[k] = g.normal(0.0, sd.get(k, 1.0), size=shapes[k]).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _scaled_params(decoder, d, m, n, r, wscale, ascale):
    p = dict(_generic_params(decoder, d, m, n, r))
    for k, f in (("W", wscale), ("Wb", wscale), ("A", ascale), ("Ab", ascale)):
        p[k] = (p[k] * np.float32(f)).astype(np.float32)
    return p


def generic_params(c):
    """fp32 parameters (as float32 arrays; do not modify): W ~ N(0, 0.6), A ~ N(0, r^-1/2),
    everything else N(0, 1), one RandomState(13) stream in parameter order; in the saturated
    regime the same stream with W, Wb and A, Ab scaled (rounded once to float32)."""
    if c.get("regime", "generic") == "generic":
        return _generic_params(c["dec"], c["d"], c["m"], c["n"], c["r"])
    return _scaled_params(c["dec"], c["d"], c["m"], c["n"], c["r"], c["wscale"], c["ascale"])


def _p64(c):
    return {k: v.astype(np.float64) for k, v in generic_params(c).items()}


# --------------------------------------------------------------------------------------------
# references of one step
# --------------------------------------------------------------------------------------------
def _batch(c, b):
    data, neg1, neg2 = case_dataset(c)
    xs = data.split["train"]
    rows = slice(b * c["l"], (b + 1) * c["l"])
    return xs.xFeats[rows], xs.args1[rows], xs.args2[rows], neg1[:, rows], neg2[:, rows]


def softmax_form(c):
    """The oracle's softmax backward for the case's regime: saturated cases take the pairwise
    form for W and Wb (the direct one is 2.7e-5 off in rho there, 9e-15 at generic parameters)."""
    return "pairwise" if c.get("regime", "generic") == "saturated" else "direct"


def oracle_step(c, b, bf16=False, params=None, **override):
    """rae_oracle.train_step_grads (float64) on batch b of the case: (cost, grads)."""
    X, e1, e2, n1, n2 = _batch(c, b)
    hp = dict(alpha=c["alpha"], lambda1=c["l1"], lambda2=c["l2"], adjust=c["l"] / c["N"],
              ext_reg=c["ext_reg"], softmax_backward=softmax_form(c))
    hp.update(override)
    res = O.train_step_grads(c["dec"], _p64(c) if params is None else params,
                             X.astype(np.float64), e1, e2, n1, n2, bf16=bf16, **hp)
    return res.cost, res.grads


def centred32_step(c, b):
    """The second float32 host: the oracle's step evaluated in numpy float32 with the centred
    softmax backward the kernels document (rae_oracle.softmax_backward_centred):
    (cost, grads as float64 arrays)."""
    X, e1, e2, n1, n2 = _batch(c, b)
    p = {k: np.asarray(v, dtype=np.float32) for k, v in generic_params(c).items()}
    res = O.train_step_grads(c["dec"], p, X.astype(np.float32), e1, e2, n1, n2, alpha=c["alpha"],
                             lambda1=c["l1"], lambda2=c["l2"], adjust=c["l"] / c["N"],
                             ext_reg=c["ext_reg"], softmax_backward="centred")
    assert all(g.dtype == np.float32 for g in res.grads.values())
    return float(res.cost), {k: g.astype(np.float64) for k, g in res.grads.items()}


def saturation(c, b):
    """How saturated batch b's inputs are (float64): the share of scores with |u| > U_SAT (from
    the oracle's log sigmoids: below -87, or within e^-87 of 0) and with |u| > U_LIN, the share
    of shifted logits z = S - max S below Z_SAT, the largest logit gap."""
    X, e1, e2, n1, n2 = _batch(c, b)
    p = _p64(c)
    res = O.train_step_grads(c["dec"], p, X.astype(np.float64), e1, e2, n1, n2, alpha=c["alpha"])
    l, s = c["l"], c["s"]
    ls = np.concatenate([res.scores[:2 * l], res.scores[4 * l:]])
    big = (ls < -U_SAT) | (ls > -math.exp(-U_SAT))
    lin = (ls < -U_LIN) | (ls > -math.log1p(math.exp(-U_LIN)))
    S = O.encoder_forward(X.astype(np.float64), p["W"], p["Wb"])[0]
    z = S - S.max(axis=1, keepdims=True)
    return dict(u=float(big.mean()), u16=float(lin.mean()), z=float((z < Z_SAT).mean()), gap=float(-z.min()))


def autograd_step(c, b, dtype=torch.float64):
    """cpu_ref.cost_graph under torch autograd in `dtype`, plus the regulariser
    adjust (lambda1 sum|w| + lambda2 sum w^2) over rae_oracle.reg_names: (cost, grads)."""
    X, e1, e2, n1, n2 = _batch(c, b)
    names = O.param_names(c["dec"])
    p = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in generic_params(c).items()}
    Xt = cpu_ref.batch_csr(X, slice(None), dtype)
    ix = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64))
    cost = cpu_ref.cost_graph(c["dec"], p, Xt, ix(e1), ix(e2), ix(n1), ix(n2), c["alpha"])
    if c["l1"] != 0.0 or c["l2"] != 0.0:
        adjust = c["l"] / c["N"]
        for k in O.reg_names(c["dec"], c["ext_reg"]):
            cost = cost + adjust * (c["l1"] * p[k].abs().sum() + c["l2"] * p[k].square().sum())
    grads = torch.autograd.grad(cost, [p[k] for k in names])
    out = {}
    for k, gk in zip(names, grads):
        gk = gk.to_dense() if gk.is_sparse else gk
        out[k] = gk.detach().double().numpy()
    return float(cost.detach().double()), out


_REFS = {}


def references(c, b):
    """The references of batch b, computed once per (dataset, decoder, shape, option):
    dict(cost64, g64, cost32, g32, rho32 [, cost_emu, g_emu, rho_emu])."""
    key = (c["dec"], c["m"], c["r"], c["s"], c["l"], c["d"], c["hot"], c["option"], c["bf16"], b,
           c["regime"], c["wscale"], c["ascale"], c["kappa"])
    if key not in _REFS:
        kappa = c["kappa"]
        cost64, g64 = oracle_step(c, b)
        cost32, g32 = autograd_step(c, b, torch.float32)
        ref = dict(cost64=cost64, g64=g64, cost32=cost32, g32=g32,
                   rho32={k: rho(g32[k], g64[k], kappa) for k in g64})
        if c["regime"] == "saturated":
            # the yardstick of a tensor is the better of the two float32 hosts
            ref["cost32c"], ref["g32c"] = centred32_step(c, b)
            ref["rho32a"] = ref["rho32"]
            ref["rho32c"] = {k: rho(ref["g32c"][k], g64[k], kappa) for k in g64}
            ref["rho32"] = {k: min(ref["rho32a"][k], ref["rho32c"][k]) for k in g64}
            ref["sat"] = saturation(c, b)
        if c["bf16"]:
            ref["cost_emu"], ref["g_emu"] = oracle_step(c, b, bf16=True)
            ref["rho_emu"] = {k: rho(ref["g_emu"][k], g64[k], kappa) for k in g64}
        _REFS[key] = ref
    return _REFS[key]


# --------------------------------------------------------------------------------------------
# metric, tolerance, extraction
# --------------------------------------------------------------------------------------------
def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(1, -1) if x.ndim == 1 else x.reshape(-1, x.shape[-1])


def row_max(g):
    """max |g| of every row (rows along the last axis; a vector is one row), shaped to
    broadcast against g."""
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 1:
        return np.full(g.shape, np.abs(g).max(initial=0.0))
    return np.broadcast_to(np.abs(g).max(axis=-1, keepdims=True), g.shape)


def rho(x, g, kappa=0.0):
    """max |x - g| / rowmax |g| over the rows where g is not identically zero; where a row of
    g is exactly zero x must be exactly zero (inf otherwise).  kappa > 0 (the saturated regime):
    the denominator of a row is max(rowmax |g|, kappa max |g| over the tensor)."""
    x2, g2 = _rows(x), _rows(g)
    rm = np.abs(g2).max(axis=1)
    zero = rm == 0.0
    if np.any(x2[zero] != 0.0):
        return math.inf
    if zero.all():
        return 0.0
    den = rm[~zero] if kappa == 0.0 else np.maximum(rm[~zero], kappa * rm.max())
    return float((np.abs(x2 - g2).max(axis=1)[~zero] / den).max())


def row_den(g, kappa=0.0):
    """rho's denominator of every element (row_max, floored at kappa max |g| over the tensor)."""
    rm = row_max(g)
    return rm if kappa == 0.0 else np.maximum(rm, kappa * np.abs(g).max(initial=0.0))


def underflow_share(g):
    """The share of a gradient's non-zero elements with |g| < 2^-63: their square is below the
    smallest normal float32, so an AdaGrad accumulator may hold 0 for them and only their
    magnitude (against the row's scale) is compared -- extract_adagrad never asks their sign,
    they are far below its 1e-11."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    nz = g > 0.0
    return float((g[nz] < G2_MIN).mean()) if nz.any() else 0.0


def tolerance(rho32):
    """The fp32 tolerance on rho for a tensor whose float32 host gradient is rho32 from float64."""
    return FACTOR * max(rho32, FLOOR)


def extract_adagrad(p0, p1, acc, g_ref, tol, kappa=0.0):
    """The gradient a device AdaGrad step from a zero accumulator applied: |g| = sqrt(acc) (one
    fp32 rounding of g^2), the sign from p0 - p1 wherever |g_ref| > max(tol rowmax|g_ref|, 1e-11)
    (from 1e-11 up the step is at least 1e-6: more than an ulp of any |p| < 8); elsewhere only
    the magnitude is compared, i.e. the reference's sign is taken.  kappa: rho's floor on the
    row's denominator."""
    p0, p1, acc, g_ref = (np.asarray(v, dtype=np.float64) for v in (p0, p1, acc, g_ref))
    need = np.abs(g_ref) > np.maximum(tol * row_den(g_ref, kappa), 1e-11)
    sgn = np.where(need, np.sign(p0 - p1), np.where(g_ref < 0, -1.0, 1.0))
    return sgn * np.sqrt(acc)


def emulate_opt_update(p, acc, g, lr, opt):
    """csrc/rae_common.hpp opt_update in numpy float32: (p', acc')."""
    p, acc, g = (np.asarray(v, dtype=np.float32) for v in (p, acc, g))
    lr = np.float32(lr)
    if opt == "adagrad":
        a = (acc + g * g).astype(np.float32)
        step = ((lr * g).astype(np.float32) / (np.sqrt(a) + np.float32(1e-6))).astype(np.float32)
        return (p - step).astype(np.float32), a
    # SGD: one rounding of p - lr g (an fma)
    return (p.astype(np.float64) - np.float64(lr) * g.astype(np.float64)).astype(np.float32), acc


# --------------------------------------------------------------------------------------------
# the assertions of one step (tests/test_gpu_options.py, tests/test_gpu_dp_options.py; on the
# CPU tests/test_grad_ref.py feeds them planted states)
# --------------------------------------------------------------------------------------------
COST_RTOL = 2e-5            # tests/test_gpu_train.py
BF16_EXACT_FACTOR, BF16_EMU_FACTOR = 1.25, 0.25     # tests/test_gpu_fullscale.py
G = sys.modules[__name__]   # the names below are written as the tests write them


def _check_step(c, b, cost, p1, acc, tag, bad):
    """The assertions of one batch; failures are appended to `bad` (so every ratio of the case
    is printed before the test fails).  Saturated cases: rho with the KAPPA floor, the yardstick
    the better of the two float32 hosts, everything finite, and the batch really saturated."""
    ref = G.references(c, b)
    p0 = G.generic_params(c)
    lr = c["lr"]
    kappa = c["kappa"]
    sat = c["regime"] == "saturated"
    want = ref["cost64"]
    if c["bf16"]:
        dc = abs(ref["cost_emu"] - want)
        ok = (abs(cost - want) <= BF16_EXACT_FACTOR * dc + COST_RTOL * abs(want) and
              abs(cost - ref["cost_emu"]) <= BF16_EMU_FACTOR * dc + COST_RTOL * abs(want))
    else:
        ok = abs(cost - want) <= COST_RTOL * max(1.0, abs(want))
    print(f"COST {tag} b{b} gpu {cost:.9g} oracle {want:.9g} rel {abs(cost - want) / abs(want):.2e}")
    if not ok:
        bad.append(f"b{b} cost {cost!r} oracle {want!r}")
    if sat:
        st = ref["sat"]
        print(f"SAT {tag} b{b} |u|>{U_SAT:g} {st['u']:.4f} |u|>{U_LIN:g} {st['u16']:.4f} "
              f"z<{Z_SAT:g} {st['z']:.4f} gap {st['gap']:.1f}")
        # at A, Ab x 2 no decoder score reaches +-87 (max |u| is 10 ... 20: the share is printed
        # only); the "saturated-scores" cases are there for that
        if c["scores"] and not (st["u"] > 0.0 and st["u16"] > st["u"]):
            bad.append(f"b{b} inputs: no score beyond {U_SAT} / {U_LIN}")
        if c["wscale"] == SAT_W_DEFAULT and not st["z"] > 0.0:
            bad.append(f"b{b} inputs: no shifted logit below {Z_SAT}")
        if not math.isfinite(cost):
            bad.append(f"b{b} cost is not finite")
        for k in p1:
            if not (np.all(np.isfinite(p1[k])) and (k not in acc or np.all(np.isfinite(acc[k])))):
                bad.append(f"b{b} {k}: state is not finite")
    for k, g64 in ref["g64"].items():
        t = G.tolerance(ref["rho32"][k])
        emu = ref["rho_emu"][k] if c["bf16"] else 0.0
        tol_exact = BF16_EXACT_FACTOR * emu + t
        a0 = p0[k].astype(np.float64)
        a1 = p1[k].astype(np.float64)
        rm = G.row_max(g64)
        # rows with an exactly zero gradient: never written
        zero = rm == 0.0
        if not np.array_equal(p1[k][zero], p0[k][zero]):
            bad.append(f"b{b} {k}: an untouched row changed")
        if c["opt"] == "adagrad":
            ak = acc[k].astype(np.float64)
            if np.any(ak[zero] != 0.0):
                bad.append(f"b{b} {k}: accumulator of an untouched row is not zero")
            g = G.extract_adagrad(a0, a1, ak, g64, tol_exact, kappa)
            # the step's size from the accumulator alone (its sign is in g, checked by rho)
            step = lr * np.sqrt(ak) / (np.sqrt(ak) + 1e-6)
            off = np.abs(np.abs(a0 - a1) - step)
            if not np.all(off <= 8 * 2.0 ** -24 * (np.abs(a0) + lr)):
                bad.append(f"b{b} {k}: p1 is not the AdaGrad step of sqrt(acc): {off.max():.3e}")
            slack = 0.0
        else:
            g = (a0 - a1) / lr
            slack = 2.0 ** -23 * np.abs(a1) / lr      # the one rounding of p1
        r_gpu = _rho_slack(g, g64, slack, kappa)
        ratio = r_gpu / max(ref["rho32"][k], G.FLOOR)
        line = (f"RATIO {tag} b{b} {k:2s} rho_gpu {r_gpu:.3e} rho_host32 {ref['rho32'][k]:.3e} "
                f"ratio {ratio:.3f}")
        if sat:
            line += (f" autograd32 {ref['rho32a'][k]:.3e} centred32 {ref['rho32c'][k]:.3e} "
                     f"underflow {G.underflow_share(g64):.4f}")
        if c["bf16"]:
            if c["opt"] == "adagrad":       # the sign rule against this reference's own tolerance
                g = G.extract_adagrad(a0, a1, ak, ref["g_emu"][k], BF16_EMU_FACTOR * emu + t,
                                      kappa)
            r_emu = _rho_slack(g, ref["g_emu"][k], slack, kappa)
            line += f" rho_emu {emu:.3e} rho_gpu_emu {r_emu:.3e}"
            if not r_emu <= BF16_EMU_FACTOR * emu + t:
                bad.append(f"b{b} {k}: rho(gpu, emu) {r_emu:.3e} > 0.25 * {emu:.3e} + {t:.3e}")
        print(line)
        if not r_gpu <= tol_exact:
            bad.append(f"b{b} {k}: rho(gpu, f64) {r_gpu:.3e} > {tol_exact:.3e} "
                       f"(host32 {ref['rho32'][k]:.3e}, ratio {ratio:.2f})")


def _rho_slack(x, g, slack, kappa=0.0):
    """rho(x, g) with a per-element allowance `slack` taken off |x - g| first (SGD: the rounding
    of p1, which is not the gradient's error)."""
    if np.isscalar(slack):
        return G.rho(x, g, kappa)
    err = np.maximum(np.abs(x - g) - slack, 0.0)
    zero = G.row_max(g) == 0.0
    if np.any(np.asarray(x)[zero] != 0.0):
        return float("inf")
    return G.rho(g + err, g, kappa)
